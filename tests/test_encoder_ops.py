"""Encoder hot-path ops: oracle pinned to the reference's golden vectors (CPU), and the gfx950
kernels (transplat_amd.kernels, called through the C-ABI) against the oracle (GPU).

Tolerances: the window attention runs exact-fp32 MFMA but with a different summation order and
exp2-based softmax than torch: 2e-4 absolute on O(1) outputs. The correlation kernels sum 128
products in a different order than MSDA+mean: 1e-4 absolute (outputs are O(1)).
"""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from canonical import seeded  # noqa: E402

from oracle import encoder_ops as E  # noqa: E402
from transplat_amd import synthetic as S  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"


def _cams(b, hw, depths=128):
    """(v b)-ordered pixel intrinsics, relative poses and `depths` disparities as the reference's
    prepare_feat_proj_data_lists builds them for the synthetic context views; hw: one side of a
    square map, or (h, w) for the native intrinsics of a non-square one."""
    from transplat_amd.model.encoder.matching.depth_predictor_trans import prepare_feat_proj_data_lists

    h, w = hw if isinstance(hw, tuple) else (hw, hw)
    ctx = S.make_batch(b, image_shape=(h, w))["context"]
    feats = torch.zeros((b, 2, 1, h, w))
    _, intr, poses, disp = prepare_feat_proj_data_lists(feats, ctx["intrinsics"], ctx["extrinsics"], ctx["near"],
                                                        ctx["far"], depths)
    return intr, poses[0], disp.flatten(1)


# ------------------------------------------------------------------ oracle vs reference golden
@pytest.mark.parametrize("shift", [0, 1])
def test_oracle_window_attention_matches_reference(shift):
    g = np.load(GOLD / "win_attn.npz")
    h = w = 16
    q, k, v = seeded((2, h * w, 128), 101), seeded((2, h * w, 128), 102), seeded((2, h * w, 128), 103)
    np.testing.assert_allclose(E.window_attention(q, k, v, h, w, 2, bool(shift)).numpy(), g[f"o2_shift{shift}"],
                               atol=1e-5)
    k4, v4 = seeded((2, 2, h * w, 128), 104), seeded((2, 2, h * w, 128), 105)
    np.testing.assert_allclose(E.window_attention(q, k4, v4, h, w, 2, bool(shift)).numpy(), g[f"o3_shift{shift}"],
                               atol=1e-5)


def test_oracle_calculate_grid_matches_reference():
    g = np.load(GOLD / "calc_grid.npz")
    grid = E.calculate_grid(torch.tensor(g["intr"]), torch.tensor(g["pose"]), torch.tensor(g["disp"]), 16, 16)
    np.testing.assert_allclose(grid.numpy(), g["grid"], atol=1e-5)


def test_camera_prep_matches_reference_golden():
    """prepare_feat_proj_data_lists restatement == the reference's (intr, pose, disp)."""
    g = np.load(GOLD / "calc_grid.npz")
    intr, pose, disp = _cams(1, 16)
    np.testing.assert_allclose(intr.numpy(), g["intr"], rtol=1e-6)
    np.testing.assert_allclose(pose.numpy(), g["pose"], atol=1e-6)
    np.testing.assert_allclose(disp.numpy(), g["disp"], rtol=1e-6)


# ------------------------------------------------------------------ HIP kernels vs oracle
def _map_hw(hw):
    """(h, w) of a map given as one side (square) or as an (h, w) pair"""
    return hw if isinstance(hw, tuple) else (hw, hw)


# 32 x 96 in 2 x 2 windows: window width 48 (no power of two) on a non-square map, key split 4 -- every
# shared geometry function takes its division path
WIDE = (32, 96)
WINATTN_CASES = [(16, 1, False, 2), (16, 1, True, 2), (16, 2, True, 2), (64, 1, False, 2), (64, 1, True, 2),
                 (64, 2, True, 2), (32, 2, False, 2), (64, 1, True, 8), (64, 1, True, 1), (64, 1, False, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("hw,m,shift,b,variant",
                         [(*c, v) for v in ("auto", "16") for c in WINATTN_CASES]
                         + [pytest.param(WIDE, 1, True, 1, "auto", id="32x96-1-True-1-auto")])
def test_window_attention_kernel(device, monkeypatch, hw, m, shift, b, variant):
    """auto: 128-query blocks as 4 waves x 32 queries (32x32x2) with the global key split + combine
    (b = 1 / 2 at 64x64, b = 1 at 32x96), without split at b = 8, the 64-query 16x16x4 kernel for 8x8
    windows; "16": the 64-query 16x16x4 kernel forced (TSPLAT_WINATTN=16) at every shape."""
    from transplat_amd import kernels as K

    if variant != "auto":
        monkeypatch.setenv("TSPLAT_WINATTN", variant)
    h, w = _map_hw(hw)
    q = seeded((b, h * w, 128), 11)
    k = seeded((b, m, h * w, 128), 12) if m > 1 else seeded((b, h * w, 128), 12)
    v = seeded(k.shape, 13)
    ref = E.window_attention(q, k, v, h, w, 2, shift)
    out = K.window_attention(q.to(device), k.to(device), v.to(device), h, w, 2, shift).cpu()
    err = (out - ref).abs().max().item()
    assert err < 2e-4, err


@pytest.mark.gpu
def test_window_attention_kernel_large_logits(device):
    """Scores far from 0 (online-softmax rescaling path exercised: later key tiles raise the max)."""
    from transplat_amd import kernels as K

    hw = 32
    q = seeded((1, hw * hw, 128), 21) * 3
    k = seeded((1, hw * hw, 128), 22) * 3
    k[:, -64:] *= 4  # the last key tile of every window holds the largest scores
    v = seeded((1, hw * hw, 128), 23)
    ref = E.window_attention(q, k, v, hw, hw, 2, True)
    out = K.window_attention(q.to(device), k.to(device), v.to(device), hw, hw, 2, True).cpu()
    assert (out - ref).abs().max().item() < 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize("hw,b,variant", [(16, 1, "dedup"), (32, 2, "dedup"), (64, 1, "dedup"), (64, 2, "dedup"),
                                          (16, 1, "direct"), (64, 1, "direct"), (16, 1, "bitmap"),
                                          (64, 2, "bitmap"), (64, 2, "run6")])
def test_uv_coarse_kernel(device, monkeypatch, hw, b, variant):
    """Run-deduplicated coarse correlation (default; run6: its 6-wave form, TSPLAT_CORR_RUN_WPE=6),
    the round-2 bitmap kernel (TSPLAT_UV_COARSE_BITMAP=1) and the sample-then-dot kernel
    (TSPLAT_UV_COARSE_DIRECT=1), incl. the production 64 x 64 map at b = 1 and 2."""
    from transplat_amd import kernels as K

    if variant == "direct":
        monkeypatch.setenv("TSPLAT_UV_COARSE_DIRECT", "1")
    if variant == "bitmap":
        monkeypatch.setenv("TSPLAT_UV_COARSE_BITMAP", "1")
    if variant == "run6":  # the run kernel at the 6-wave register budget (two dot passes in flight)
        monkeypatch.setenv("TSPLAT_CORR_RUN_WPE", "6")
    intr, pose, disp = _cams(b, hw)
    feat = seeded((b, 2, hw * hw, 128), 31)
    ref = E.uv_coarse(feat, intr, pose, disp, hw, hw)
    out = K.uv_coarse(feat.to(device), intr.to(device), pose.to(device), disp.to(device), hw, hw).cpu()
    assert (out - ref).abs().max().item() < 1e-4


def _rotated_cams(b, hw, seed, depth_slice=lambda d: d, depths=128):
    """_cams with the relative pose turned by a random rotation of up to ~0.35 rad and shifted, so
    epipolar segments run diagonally, leave the image and re-enter the sampling window part-way,
    and the depth count is changed (S = 1, 3 slices of 64 samples)."""
    intr, pose, disp = _cams(b, hw, depths)
    g = torch.Generator().manual_seed(seed)
    pose = pose.clone()
    for i in range(pose.shape[0]):
        w = (torch.rand(3, generator=g) - 0.5) * 0.7
        th = w.norm()
        kx = torch.tensor([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]) / th
        rot = torch.eye(3) + torch.sin(th) * kx + (1 - torch.cos(th)) * kx @ kx
        pose[i, :3, :3] = rot @ pose[i, :3, :3]
        pose[i, :3, 3] += (torch.rand(3, generator=g) - 0.5) * 0.6
    return intr, pose, depth_slice(disp).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,depths", [(1, 128), (2, 64), (3, 192)])
def test_uv_coarse_run_matches_bitmap(device, monkeypatch, seed, depths):
    """The run-deduplicated kernel equals the bitmap kernel BIT FOR BIT (same distinct-corner dots,
    same per-sample sum order, sample positions from the same contraction-free sample_im) on
    rotated cameras with D = 64 / 128 / 192, and holds the oracle's 1e-4."""
    from transplat_amd import kernels as K

    sl = {128: lambda d: d, 64: lambda d: d[:, ::2], 192: lambda d: torch.cat([d, d[:, ::2] * 1.003], 1)}[depths]
    hw = 32
    intr, pose, disp = _rotated_cams(2, hw, seed, sl)
    assert disp.shape[1] == depths
    feat = seeded((2, 2, hw * hw, 128), 40 + seed)
    args = (feat.to(device), intr.to(device), pose.to(device), disp.to(device), hw, hw)
    run = K.uv_coarse(*args).cpu()
    monkeypatch.setenv("TSPLAT_UV_COARSE_BITMAP", "1")
    bitmap = K.uv_coarse(*args).cpu()
    ref = E.uv_coarse(feat, intr, pose, disp, hw, hw)
    d_bitmap, d_ref = (run - bitmap).abs().max().item(), (run - ref).abs().max().item()
    print(f"coarse run kernel seed={seed} D={depths}: vs bitmap kernel {d_bitmap:.2e} "
          f"({(run != bitmap).float().mean().item():.2e} of outputs differ), vs oracle {d_ref:.2e}")
    assert d_bitmap == 0 and d_ref < 1e-4
    assert (ref != 0).float().mean().item() > 0.1  # the segments do cross the image


@pytest.mark.gpu
@pytest.mark.parametrize("hw,b,variant", [(16, 1, "table"), (24, 2, "table"), (64, 1, "table"), (16, 1, "direct"),
                                          (24, 2, "direct"), (24, 2, "table_bf16"), (64, 1, "table_bf16"),
                                          (24, 2, "table_bf16x3"), (64, 1, "table_bf16x3")])
def test_uv_cross_kernel(device, hw, b, variant):
    """Both forms of the fine cross correlation: the correlation-table gather (default) and the
    direct feature-row sampling kernel; table_bf16: a bf16 value (bf16 dense mode, the value_proj
    output) takes the split-bf16 table GEMM (key = hi + lo bf16 halves, fp32 accumulate), checked
    against the fp32 restatement on the same bf16-exact values; table_bf16x3: fp32 key and value in
    the bf16x3 dense mode (both split, one K = 3C bf16 GEMM), at the same 1e-4 bound."""
    import contextlib

    from transplat_amd import kernels as K

    op = K.uv_cross if variant != "direct" else K.uv_cross_direct
    intr, pose, disp = _cams(b, hw)
    value = seeded((b, 2, hw * hw, 128), 41)
    if variant == "table_bf16":
        value = value.bfloat16()
    key = seeded((b, 2, hw * hw, 128), 42)
    offsets = seeded((b * 2, hw * hw, 128 * 4 * 2), 43, 2.0)
    logits = seeded((b * 2, hw * hw, 128 * 4), 44)
    ref = E.uv_cross(value.float(), key, intr, pose, disp, offsets, logits, hw, hw)
    mode = K.dense_precision("bf16x3") if variant == "table_bf16x3" else contextlib.nullcontext()
    with mode:
        out = op(*(t.to(device) for t in (value, key, intr, pose, disp, offsets, logits)), hw, hw).cpu()
    assert (out - ref).abs().max().item() < 1e-4


@pytest.mark.gpu
def test_msda_kernel(device):
    from transplat_amd import kernels as K

    hw = 16
    value = seeded((2, hw * hw, 128), 51)
    loc = seeded((2, hw * hw, 4, 2), 52, kind="rand") * 1.2 - 0.1  # some samples off-image
    wts = torch.softmax(seeded((2, hw * hw, 4), 53), -1)
    ref = E.msda(value, loc, wts, hw, hw)
    out = K.msda(value.to(device), loc.to(device), wts.to(device), hw, hw).cpu()
    assert (out - ref).abs().max().item() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("b,v", [(1, 2), (2, 3)])
def test_depth_tail_kernel(device, b, v):
    """tsplat_depth_tail_fwd (1 / clamp(fullres + delta, 1 / far, 1 / near) and sigmoid, written in
    the (b v) layout) against the reference's operations (oracle.depth_tail), incl. values clamped
    at both ends and the (v b) -> (b v) reorder at b > 1."""
    from transplat_amd import kernels as K

    h, w = 12, 20
    fullres = seeded((v * b, 1, h, w), 61, kind="rand") * 0.5 + 0.02
    head = seeded((v * b, 2, h, w), 62) * 0.3
    near = seeded((b, v), 63, kind="rand") + 0.5
    far = near + seeded((b, v), 64, kind="rand") * 50 + 5
    rd, rn = E.depth_tail(fullres, head, near, far)
    od, on = (t.cpu() for t in K.depth_tail(fullres.to(device), head.to(device), near.to(device), far.to(device)))
    assert ((rd - od).abs() / rd.abs()).max().item() < 1e-6
    assert (rn - on).abs().max().item() < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(16, 16), (12, 20)])
def test_msda_raw_kernel(device, hw):
    """tsplat_msda_raw_fwd (reference points, offset scaling and the softmax over the points in the
    kernel) against the reference's operations restated (oracle.msda_raw), incl. samples pushed off
    the map and a non-square grid; and UVSelfAttention.core_raw against core() on the same module."""
    from transplat_amd import kernels as K
    from transplat_amd.model.utils.uv_transformer import UVSelfAttention

    h, w = hw
    value = seeded((2, h * w, 128), 54)
    ow = torch.zeros((2, h * w, 128))
    ow[..., :8] = seeded((2, h * w, 8), 55) * 3.0
    ow[..., 8:12] = seeded((2, h * w, 4), 56)
    ref = E.msda_raw(value, ow, 4, h, w)
    out = K.msda_raw(value.to(device), ow.to(device), 4, h, w).cpu()
    assert (out - ref).abs().max().item() < 1e-5
    torch.manual_seed(0)
    sa = UVSelfAttention(embed_dims=128).to(device).eval()
    q, pos = seeded((2, h * w, 128), 57).to(device), seeded((2, h * w, 128), 58).to(device)
    from transplat_amd.model.utils.uv_transformer import UVTransformerEncoder

    ref2d = UVTransformerEncoder.reference_points_2d(h, w, 2, torch.float32, device)
    with torch.no_grad():
        a = sa.core(q, q, pos, ref2d, h, w)
        b = sa.core_raw(q, q, pos, h, w)
    err = (a - b).abs().max().item() / a.abs().max().item()
    print(f"msda raw vs module chain: {err:.2e}")
    assert err < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", [((6, 3, 256, 256), (252, 252)), ((2, 64, 18, 18), (64, 64)),
                                        ((16, 1, 252, 252), (256, 256)), ((3, 5, 7, 9), (13, 4)),
                                        ((2, 2, 1, 1), (3, 5)), ((2, 4, 64, 64), (256, 256))])
def test_resize_bilinear_nchw_kernel(device, shape, size):
    """tsplat_resize_bilinear_nchw_fwd (align_corners=True, any size, NCHW) vs the oracle
    (F.interpolate on the CPU, whose interpolation weights are computed differently: 2e-5 of the
    output's magnitude) and vs PyTorch's own GPU kernel, whose float arithmetic it restates (1e-6)."""
    import torch.nn.functional as F

    from transplat_amd import kernels as K

    x = seeded(shape, 33)
    ref = E.resize_bilinear_nchw(x, size)
    xd = x.to(device)
    out = K.interpolate_bilinear_ac(xd, size)
    scale = max(1.0, ref.abs().max().item())
    assert out.shape == ref.shape
    assert (out.cpu() - ref).abs().max().item() < 2e-5 * scale
    ref_gpu = F.interpolate(xd, size, mode="bilinear", align_corners=True)
    assert (out - ref_gpu).abs().max().item() < 1e-6 * scale


# ---- mmcv-shaped multi-level / multi-head MSDA (tsplat_ms_deform_attn_fwd)
def _msda_pytorch(value, shapes, loc, wts):
    """mmcv's multi_scale_deformable_attn_pytorch (grid_sample form, the published fallback the
    reference imports at src/model/utils/attention.py:8), restated as the independent check."""
    import torch.nn.functional as F

    bs, _, nh, hd = value.shape
    _, nq, _, nl, npt, _ = loc.shape
    vals = value.split([int(h) * int(w) for h, w in shapes], dim=1)
    grids = 2 * loc - 1
    outs = []
    for lvl, (h, w) in enumerate(shapes):
        v = vals[lvl].flatten(2).transpose(1, 2).reshape(bs * nh, hd, int(h), int(w))
        g = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)
        outs.append(F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False))
    a = wts.transpose(1, 2).reshape(bs * nh, 1, nq, nl * npt)
    out = (torch.stack(outs, dim=-2).flatten(-2) * a).sum(-1).view(bs, nh * hd, nq)
    return out.transpose(1, 2).contiguous()


def _msda_case(bs, nh, hd, shapes, nq, npt, seed):
    shapes_t = torch.tensor(shapes, dtype=torch.int64)
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), (shapes_t[:, 0] * shapes_t[:, 1]).cumsum(0)[:-1]])
    nk = int((shapes_t[:, 0] * shapes_t[:, 1]).sum())
    value = seeded((bs, nk, nh, hd), seed)
    loc = seeded((bs, nq, nh, len(shapes), npt, 2), seed + 1, kind="rand") * 1.3 - 0.15  # some off-map
    wts = torch.softmax(seeded((bs, nq, nh, len(shapes) * npt), seed + 2), -1).reshape(bs, nq, nh, len(shapes), npt)
    return value, shapes_t, starts, loc, wts


MSDA_CASES = [  # bs, heads, head dim, level shapes, queries, points
    (2, 8, 32, [(16, 16), (8, 8), (4, 4), (2, 2)], 50, 4),  # deformable-DETR style
    (1, 1, 128, [(16, 16)], 256, 4),                        # TranSplat's UV self-attention shape
    (3, 2, 6, [(7, 5), (3, 9)], 33, 3),                     # head dim not a multiple of 4, ragged maps
]


@pytest.mark.parametrize("case", MSDA_CASES)
def test_oracle_ms_deform_attn_matches_mmcv_pytorch(case):
    value, shapes, starts, loc, wts = _msda_case(*case, seed=71)
    ref = _msda_pytorch(value, shapes, loc, wts)
    out = E.ms_deform_attn(value, shapes, starts, loc, wts)
    assert (out - ref).abs().max().item() < 1e-5


def test_oracle_ms_deform_attn_single_level_is_msda():
    value, shapes, starts, loc, wts = _msda_case(2, 1, 128, [(12, 12)], 40, 4, seed=75)
    a = E.ms_deform_attn(value, shapes, starts, loc, wts)
    b = E.msda(value[:, :, 0], loc[:, :, 0, 0], wts[:, :, 0, 0], 12, 12)
    assert (a - b).abs().max().item() < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("case", MSDA_CASES)
def test_ms_deform_attn_kernel(device, case):
    from transplat_amd.model.utils.multi_scale_deformable_attn_function import MultiScaleDeformableAttnFunction_fp32

    value, shapes, starts, loc, wts = _msda_case(*case, seed=81)
    ref = E.ms_deform_attn(value, shapes, starts, loc, wts)
    out = MultiScaleDeformableAttnFunction_fp32.apply(*(t.to(device) for t in (value, shapes, starts, loc, wts)), 64)
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert (out.cpu() - ref).abs().max().item() < 1e-5


@pytest.mark.gpu
def test_ms_deform_attn_level_start_index_and_im2col_step(device):
    """Levels are read from level_start_index (not re-derived from the shapes), and the batch must
    be divisible by min(batch, im2col_step) as mmcv asserts."""
    from transplat_amd import kernels as K

    value, shapes, starts, loc, wts = _msda_case(4, 2, 8, [(6, 6), (3, 3)], 20, 2, seed=85)
    # the same levels stored in the opposite order in value
    a, b = value[:, :36], value[:, 36:]
    swapped = torch.cat([b, a], 1)
    starts2 = torch.tensor([9, 0], dtype=torch.int64)
    ref = E.ms_deform_attn(value, shapes, starts, loc, wts)
    out = K.ms_deform_attn(*(t.to(device) for t in (swapped, shapes, starts2, loc, wts)), im2col_step=2)
    assert (out.cpu() - ref).abs().max().item() < 1e-5
    with pytest.raises(RuntimeError, match="invalid argument"):
        K.ms_deform_attn(*(t.to(device) for t in (value, shapes, starts, loc, wts)), im2col_step=3)


def _adapter_inputs(b=2, v=2, h=24, w=32, d_sh=25):
    raw = seeded((b, v, h * w, 9 + 3 * d_sh), 61)
    depths = 1.0 + 20 * seeded((b, v, h * w), 62, kind="rand")
    dens = seeded((b, v, h * w), 63, kind="rand")
    ctx = S.make_batch(b, image_shape=(h, w))["context"]
    ext = ctx["extrinsics"].clone()
    ext[:, 1, :3, :3] = torch.tensor([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])  # non-trivial rotation
    return raw, depths, dens, ext, ctx["intrinsics"]


def test_oracle_adapter_shapes_and_identity_rotation():
    raw, depths, dens, ext, K = _adapter_inputs(b=1, v=1)
    ext = torch.eye(4)[None, None]
    m, c, hsh, o = E.gaussian_adapter(raw, depths, dens, ext, K[:, :1], (24, 32), 0.5, 15.0)
    assert m.shape == (1, 768, 3) and c.shape == (1, 768, 3, 3) and hsh.shape == (1, 768, 3, 25)
    assert torch.allclose(o, dens.reshape(1, -1))  # map_pdf_to_opacity is the identity at exponent 1
    assert torch.allclose(c, c.transpose(-1, -2), atol=1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,b", [("bvhwc", 2), ("head_nchw", 2), ("head_nchw", 1)])
def test_gaussian_adapter_kernel(device, layout, b):
    from einops import rearrange
    from transplat_amd import kernels as K

    raw, depths, dens, ext, intr = _adapter_inputs(b=b)
    ref = E.gaussian_adapter(raw, depths, dens, ext, intr, (24, 32), 0.5, 15.0, 2.0)
    raw_d = raw.to(device)
    if layout == "head_nchw":
        # the depth head's output map [(v b), c, h, w] and the view the encoder hands the adapter
        head = rearrange(raw_d, "b v (h w) c -> (v b) c h w", h=24).contiguous()
        raw_d = rearrange(head, "(v b) c h w -> b v (h w) c", b=b)
        assert not raw_d.is_contiguous()
    out = K.gaussian_adapter(raw_d, *(t.to(device) for t in (depths, dens, ext, intr)), (24, 32), 0.5, 15.0, 2.0)
    for name, r, o in zip(("means", "cov", "harmonics", "opacity"), ref, out):
        o = o.cpu()
        # per-element relative error, floored at 1e-3 of the tensor's scale (covariances are
        # products of three fp32 terms summed in a different order than torch's matmul)
        err = ((o - r).abs() / (r.abs() + 1e-3 * r.abs().max())).max().item()
        assert err < 2e-4, (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,groups,act,res,pb", [
    ((2, 128, 64, 64), 8, "silu", False, False), ((2, 32, 256, 256), 8, "silu", True, True),
    ((2, 128, 16, 16), 8, "none", True, False), ((2, 32, 64, 64), 4, "gelu", False, True),
    ((3, 12, 5, 7), 4, "silu", True, True),  # odd HW: scalar path
    ((2, 128, 4096), 8, "none", False, True),
    ((2, 128, 64, 64), 32, "silu", True, True), ((2, 64, 32, 32), 32, "gelu", False, True),  # single launch
    ((2, 96, 40, 40), 32, "silu", True, False)])
def test_group_norm_kernel(device, shape, groups, act, res, pb):
    """GroupNorm (+ folded conv bias, + SiLU/GELU, + residual) vs torch on CPU."""
    from transplat_amd import kernels as K

    x = seeded(shape, 71) * 3 + 1.5  # non-zero mean: the Welford path matters
    w = seeded((shape[1],), 72) * 0.5 + 1
    b = seeded((shape[1],), 73) * 0.2
    r = seeded(shape, 74) if res else None
    bias = seeded((shape[1],), 75) if pb else None
    ref = E.group_norm(x, groups, w, b, 1e-5, act, r, bias)
    out = K.group_norm(x.to(device), groups, w.to(device), b.to(device), 1e-5, act,
                       r.to(device) if res else None, bias.to(device) if pb else None).cpu()
    assert (out - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    # bf16 activations (config C3): bf16 x / residual in, fp32 statistics, bf16 out -- the
    # reference's GroupNorm32 normalises x.float() and casts back; checked on the same bf16 inputs
    xb, rb = x.bfloat16(), (r.bfloat16() if res else None)
    ref_b = E.group_norm(xb.float(), groups, w, b, 1e-5, act, rb.float() if res else None, bias)
    out_b = K.group_norm(xb.to(device), groups, w.to(device), b.to(device), 1e-5, act,
                         rb.to(device) if res else None, bias.to(device) if pb else None)
    assert out_b.dtype == torch.bfloat16
    # one bf16 rounding of the output (2^-8 relative) on top of fp32 arithmetic
    assert (out_b.float().cpu() - ref_b).abs().max().item() < 8e-3 * max(1.0, ref_b.abs().max().item())
    if res:
        # an fp32 residual beside a bf16 x (an identity skip of an fp32 stream): the module path's
        # bf16(norm) + fp32 residual, promoted to fp32 -- the residual is not narrowed to bf16
        out_m = K.group_norm(xb.to(device), groups, w.to(device), b.to(device), 1e-5, act, r.to(device),
                             bias.to(device) if pb else None)
        assert out_m.dtype == torch.float32
        ref_m = E.group_norm(xb.float(), groups, w, b, 1e-5, act, None, bias).bfloat16().float() + r
        assert (out_m.cpu() - ref_m).abs().max().item() < 8e-3 * max(1.0, ref_m.abs().max().item())


@pytest.mark.gpu
def test_sh_rotation_op_matches_oracle(device):
    from transplat_amd import kernels as K

    _, _, _, ext, _ = _adapter_inputs()
    rot = ext[..., :3, :3].reshape(-1, 3, 3)
    ref = E.sh_rotation(rot, 25)
    out = K.sh_rotation(rot.to(device), 25).cpu()
    assert (out - ref).abs().max().item() < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("hw,m,shift,b,grow", [(64, 1, False, 2, False), (64, 1, True, 2, False), (64, 2, True, 2, False),
                                               (32, 1, True, 2, False), (64, 1, True, 8, False), (64, 1, True, 1, False),
                                               (64, 1, True, 2, True), (64, 1, False, 1, True),
                                               pytest.param(WIDE, 1, True, 1, False, id="32x96-1-True-1-False")])
def test_window_attention_x3_kernel(device, hw, m, shift, b, grow):
    """bf16x3 window attention (tsplat_win_attn_x3_fwd: split-bf16 products, fp32 softmax; the C2
    step's dense-precision mode) vs the oracle in float64, relative to max(1, max |O|): within 3e-5
    on O(1) scores (the exact-fp32 kernel's bound is 2e-4), and in every case within 1/8 of the error
    of TF32-rounded q / k / v (the reference's own GPU arithmetic rounds those operands and P too).
    grow: scores that keep rising along the keys (the deferred-rescale path, P up to 2^8), |s| up to
    ~10^2 -- the score error scales with the logits (measured 5.6e-5 there), hence 2e-4."""
    from transplat_amd import kernels as K

    h, w = _map_hw(hw)
    q = seeded((b, h * w, 128), 51) * (3.0 if grow else 1.0)
    k = seeded((b, m, h * w, 128), 52) if m > 1 else seeded((b, h * w, 128), 52)
    if grow:
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        t = ((ys % (h // 2)) * (w // 2) + xs % (w // 2)).reshape(-1).float() / (h * w / 4)
        k = k * (0.25 + 3.75 * t)[None, :, None]
    v = seeded(k.shape, 53)
    ref = E.window_attention(q.double(), k.double(), v.double(), h, w, 2, shift)
    out = K.window_attention_x3(q.to(device), k.to(device), v.to(device), h, w, 2, shift).cpu().double()
    scale = max(1.0, ref.abs().max().item())
    err = (out - ref).abs().max().item() / scale
    def tf(t):  # fp32 -> TF32 (10 explicit mantissa bits, round to nearest even)
        i = t.float().contiguous().view(torch.int32)
        return ((i + 0xFFF + ((i >> 13) & 1)) & ~0x1FFF).view(torch.float32).double()

    ref_tf = E.window_attention(tf(q), tf(k), tf(v), h, w, 2, shift)
    err_tf = (ref_tf - ref).abs().max().item() / scale
    print(f"x3 attention hw={hw} m={m} shift={shift} b={b} grow={grow}: rel err {err:.2e}, TF32 operands {err_tf:.2e}")
    assert err < (2e-4 if grow else 3e-5) and err <= err_tf / 8, (err, err_tf)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,ksplit,shift,grow", [("v1", 0, True, False), ("v1", 0, False, True),
                                                        ("v2", 1, True, False), ("v2", 2, True, True),
                                                        ("v2", 8, True, False), ("v2", 8, False, True),
                                                        ("v2s", 0, True, False), ("v2s", 2, False, True)])
def test_window_attention_x3_variants(device, monkeypatch, variant, ksplit, shift, grow):
    """The round-5 4-wave x3 kernel (TSPLAT_WINATTN_X3=v1) and the two-group kernel (default, in
    window-major XCD order; v2s: key-split-major order, TSPLAT_WINATTN_X3_XCD=split) under forced
    key splits (1: no partials, normalised output; 2 / 8: 8 / 2 key tiles per workgroup), same
    bounds as test_window_attention_x3_kernel, and the two kernels within 2e-5 of each other (they
    differ only in the running maxima the P split is taken against and the sum order)."""
    from transplat_amd import kernels as K

    hw, b = 64, 2
    q = seeded((b, hw * hw, 128), 71) * (3.0 if grow else 1.0)
    k = seeded((b, hw * hw, 128), 72)
    if grow:
        ys, xs = torch.meshgrid(torch.arange(hw), torch.arange(hw), indexing="ij")
        t = ((ys % (hw // 2)) * (hw // 2) + xs % (hw // 2)).reshape(-1).float() / (hw * hw / 4)
        k = k * (0.25 + 3.75 * t)[None, :, None]
    v = seeded(k.shape, 73)
    ref = E.window_attention(q.double(), k.double(), v.double(), hw, hw, 2, shift)
    if ksplit:
        monkeypatch.setenv("TSPLAT_WINATTN_KSPLIT", str(ksplit))
    args = (q.to(device), k.to(device), v.to(device), hw, hw, 2, shift)
    if variant == "v2s":  # the two-group kernel in key-split-major XCD order
        monkeypatch.setenv("TSPLAT_WINATTN_X3_XCD", "split")
        variant = "v2"
    monkeypatch.setenv("TSPLAT_WINATTN_X3", variant)
    out = K.window_attention_x3(*args).cpu().double()
    monkeypatch.setenv("TSPLAT_WINATTN_X3", "v1" if variant == "v2" else "v2")
    other = K.window_attention_x3(*args).cpu().double()
    scale = max(1.0, ref.abs().max().item())
    err = (out - ref).abs().max().item() / scale
    diff = (out - other).abs().max().item() / scale
    print(f"x3 {variant} ksplit={ksplit} shift={shift} grow={grow}: rel err {err:.2e}, vs the other form {diff:.2e}")
    assert err < (2e-4 if grow else 3e-5), err
    assert diff < (2e-4 if grow else 2e-5), diff


@pytest.mark.gpu
@pytest.mark.parametrize("dense", ["fp32", "bf16x3"])
@pytest.mark.parametrize("x3_from,n,m", [(1, 384, 8192), (0, 256, 8192), (1, 384, 65536)])
def test_linear_kv_x3_matches_split(device, dense, x3_from, n, m):
    """tsplat_linear_f32_split_x3_fwd (the q | k | v or k | v projection writing k / v as the bf16x3
    attention's hi / lo operand) == the fp32 split projection followed by tsplat_split_kv_bf16x3,
    bit for bit (same kernel arithmetic, the split applied to the same fp32 values); and the
    attention merge fed the pre-split operand == the one fed fp32 k / v."""
    from transplat_amd import kernels as K

    x = seeded((2, m // 2, 128), 61).to(device)
    w = (seeded((n, 128), 62) / math.sqrt(128)).to(device)
    with K.dense_precision(dense):
        ref_blocks = K.fused_linear(x, w, split=True)
        blocks, kv = K.linear_kv_x3(x, w, x3_from)
    assert len(blocks) == x3_from
    for a, b in zip(blocks, ref_blocks[:x3_from]):
        assert torch.equal(a, b)
    k, v = ref_blocks[x3_from:]
    assert torch.equal(kv, K.split_kv_bf16x3(k, v))
    if x3_from == 1 and m == 8192:
        q = blocks[0]
        wm = (seeded((128, 128), 63) / math.sqrt(128)).to(device)
        ln = (torch.ones(128, device=device), torch.zeros(128, device=device), 1e-5)
        with K.dense_precision(dense), K.attention_precision("bf16x3"):
            assert K.attention_x3_ready(2, 64, 64, 1, 2)
            a = K.attention_merge(q, k, v, 64, 64, 2, True, wm, ln, kv_shift=1)
            b = K.attention_merge(q, None, None, 64, 64, 2, True, wm, ln, kv_shift=1, kv_x3=kv)
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_window_attention_dtu_stress(device):
    """C5 stress: 3 context views at 512x384 -> a 128x96 feature map, 2 windows per side
    (L = 3072 queries, 6144 keys over two key views), shifted layer."""
    from transplat_amd import kernels as K

    h, w = 96, 128
    q = seeded((1, h * w, 128), 81)
    k = seeded((1, 2, h * w, 128), 82)
    v = seeded((1, 2, h * w, 128), 83)
    ref = E.window_attention(q, k, v, h, w, 2, True)
    out = K.window_attention(q.to(device), k.to(device), v.to(device), h, w, 2, True).cpu()
    assert (out - ref).abs().max().item() < 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["auto", "v2", "v3"])
@pytest.mark.parametrize("hw,m,shift,b", [(64, 1, False, 2), (64, 1, True, 2), (64, 2, True, 3), (32, 1, True, 16)])
def test_window_attention_bf16_kernel(device, monkeypatch, kern, hw, m, shift, b):
    """bf16 MFMA variant (config C3) vs the fp32 oracle on the same bf16-rounded inputs: P is
    rounded to bf16 for the PV product, so the bound is bf16-level (1.5e-2 absolute on O(1)
    outputs). The launch's own kernel choice and each kernel forced (TSPLAT_WINATTN_BF16: v2 =
    4 waves / 128 queries with key splits, v3 = 8 staggered waves / 256 queries)."""
    from transplat_amd import kernels as K

    if kern != "auto":
        monkeypatch.setenv("TSPLAT_WINATTN_BF16", kern)

    q = seeded((b, hw * hw, 128), 91).bfloat16()
    k = (seeded((b, m, hw * hw, 128), 92) if m > 1 else seeded((b, hw * hw, 128), 92)).bfloat16()
    v = seeded(k.shape, 93).bfloat16()
    ref = E.window_attention(q.float(), k.float(), v.float(), hw, hw, 2, shift)
    out = K.window_attention(q.to(device), k.to(device), v.to(device), hw, hw, 2, shift)
    assert out.dtype == torch.bfloat16
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < 1.5e-2, err


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["auto", "v3"])
@pytest.mark.parametrize("shift,b", [(False, 2), (True, 2), (True, 16)])
def test_window_attention_bf16_growing_scores(device, monkeypatch, kern, shift, b):
    """Scores that grow along the key order (keys scaled up to 4x, queries 3x) so the running max
    keeps moving past the bf16 kernel's deferred-rescale threshold on later key tiles (random O(1)
    scores would only take the branch on the first tile); b = 2 runs the split-key partials path,
    b = 16 the single-pass one (v3 by default); kern = v3 forces the 8-wave kernel at every b."""
    from transplat_amd import kernels as K

    if kern != "auto":
        monkeypatch.setenv("TSPLAT_WINATTN_BF16", kern)
    hw = 64
    q = (seeded((b, hw * hw, 128), 94) * 3.0).bfloat16()
    # in-window key position t of pixel (y, x) is (y % 32) * 32 + x % 32: scale by it
    ys, xs = torch.meshgrid(torch.arange(hw), torch.arange(hw), indexing="ij")
    t = ((ys % 32) * 32 + xs % 32).reshape(-1).float() / 1024.0
    k = (seeded((b, hw * hw, 128), 95) * (0.25 + 3.75 * t)[None, :, None]).bfloat16()
    v = seeded(k.shape, 96).bfloat16()
    ref = E.window_attention(q.float(), k.float(), v.float(), hw, hw, 2, shift)
    out = K.window_attention(q.to(device), k.to(device), v.to(device), hw, hw, 2, shift)
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < 1.5e-2 * max(1.0, ref.abs().max().item()), err


@pytest.mark.gpu
@pytest.mark.parametrize("shape,groups,c1", [((16, 256, 32, 32), 8, 128), ((2, 64, 64, 64), 8, 24),
                                             ((2, 96, 16, 16), 4, 64), ((3, 40, 9, 7), 4, 30),
                                             ((2, 128, 128, 128), 8, 64)])
@pytest.mark.parametrize("act", ["silu", "none"])
def test_group_norm_cat_residual(device, shape, groups, c1, act):
    """tsplat_group_norm_cat_res_fwd: the residual as a channel concatenation [r1 | r2] read in place
    (the U-Net output blocks' identity skip), bit-identical to the residual materialised by torch.cat;
    both the single-launch (small groups) and the stats + apply forms, vector and scalar (odd HW)."""
    from transplat_amd import kernels as K

    n, c = shape[:2]
    x = (seeded(shape, 76) * 2 + 0.5).to(device)
    w = (seeded((c,), 77) * 0.5 + 1).to(device)
    b = (seeded((c,), 78) * 0.2).to(device)
    pb = (seeded((c,), 79) * 0.1).to(device)
    r1 = seeded((n, c1) + shape[2:], 80).to(device)
    r2 = seeded((n, c - c1) + shape[2:], 81).to(device)
    ref = K.group_norm(x, groups, w, b, 1e-5, act, torch.cat([r1, r2], 1), pb)
    out = K.group_norm(x, groups, w, b, 1e-5, act, (r1, r2), pb)
    assert torch.equal(out, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["auto", "v2", "v3"])
@pytest.mark.parametrize("b,kvs,m", [(2, 1, 1), (8, 4, 1), (4, 3, 1), (3, 2, 2)])
def test_window_attention_bf16_kv_shift(device, monkeypatch, kern, b, kvs, m):
    """tsplat_win_attn_bf16_shift_fwd (query batch i reads the keys / values of batch (i + s) % B,
    forward_pair's cross pairing in C3) == the bf16 kernel on rolled copies of k / v, bit for bit on
    both kernels; and two identical calls agree bit for bit. (Round 5 held v2 to 4e-3 here: its
    inline-asm v_max3_f32 read the score accumulator before the MFMA had written it, so the tile max
    was now and then a partial score. The max is compiler-visible now and tests/test_isa_hazards.py
    scans every kernel for such reads.)"""
    from transplat_amd import kernels as K

    if kern != "auto":
        monkeypatch.setenv("TSPLAT_WINATTN_BF16", kern)
    hw = 64
    q = seeded((b, hw * hw, 128), 97).bfloat16().to(device)
    k = (seeded((b, m, hw * hw, 128), 98) if m > 1 else seeded((b, hw * hw, 128), 98)).bfloat16().to(device)
    v = seeded(k.shape, 99).bfloat16().to(device)
    a = K.window_attention(q, k, v, hw, hw, 2, True, kv_shift=kvs)
    ref = K.window_attention(q, torch.roll(k, -kvs, dims=0), torch.roll(v, -kvs, dims=0), hw, hw, 2, True)
    assert torch.equal(a, ref)
    for _ in range(3):
        assert torch.equal(K.window_attention(q, k, v, hw, hw, 2, True, kv_shift=kvs), a)


@pytest.mark.gpu
@pytest.mark.parametrize("dense", ["fp32", "bf16x3"])
@pytest.mark.parametrize("m,n,split,ln", [(8192, 384, True, False), (1000, 128, False, True), (65536, 256, True, False)])
def test_fused_linear_bf16_io(device, dense, m, n, split, ln):
    """fused_linear's bf16 operand / output flags (512, 1024): a bf16 x1 gives exactly the result of
    its fp32 widening, and a bf16 output is exactly the fp32 output rounded to bf16 (the C3 layer's
    q / k / v projections and bf16 message without cast launches)."""
    from transplat_amd import kernels as K

    xb = seeded((m, 128), 38).bfloat16().to(device)
    w = (seeded((n, 128), 39) / math.sqrt(128)).to(device)
    lnp = (seeded((n,), 35).to(device) * 0.1 + 1.0, seeded((n,), 36).to(device) * 0.1, 1e-5) if ln else None
    with K.dense_precision(dense):
        ref = K.fused_linear(xb.float(), w, ln=lnp, split=split)
        a = K.fused_linear(xb, w, ln=lnp, split=split)
        c = K.fused_linear(xb, w, ln=lnp, split=split, out_dtype=torch.bfloat16)
    refs, outs, outc = (ref, a, c) if split else ([ref], [a], [c])
    for r, x, y in zip(refs, outs, outc):
        assert x.dtype == torch.float32 and y.dtype == torch.bfloat16 and y.shape == r.shape
        assert torch.equal(x, r)
        assert torch.equal(y, r.to(torch.bfloat16))
    with pytest.raises(ValueError):
        K.fused_linear(xb, w, out_dtype=torch.bfloat16, residual=torch.zeros((m, n), device=device))


@pytest.mark.gpu
@pytest.mark.parametrize("m,k1,k2,n,gelu,ln,res,split,bias,gin", [
    (8192, 128, 0, 384, False, False, False, True, False, False),    # self-attention q | k | v
    (8192, 128, 0, 128, False, True, True, False, False, False),     # merge + norm1 + residual
    (1000, 128, 128, 1024, True, False, False, False, False, False),  # [x | msg] + GELU, ragged M
    (8192, 1024, 0, 128, False, True, True, False, False, True),     # GELU(h) mlp[2] + norm2 + res
    (96, 64, 0, 256, True, False, False, False, True, False),        # bias path, tiny M
    (65536, 1024, 0, 128, False, True, True, False, False, True),    # C3 b = 8: 128-row blocks (bf16x3)
    (65536, 128, 0, 384, False, False, False, True, False, False),   # C3 q | k | v, 128-row blocks
    (65500, 128, 128, 128, False, True, False, False, True, False),  # ragged M, [x | pos], LN
])
@pytest.mark.parametrize("dense", ["fp32", "bf16x3"])
def test_fused_linear_kernel(device, m, k1, k2, n, gelu, ln, res, split, bias, gin, dense):
    """tsplat_linear_f32_fwd vs the CPU restatement of the reference TransformerLayer chain
    (exact fp32 MFMA: only the summation order differs; bf16x3 mode, flag 256: split-bf16 products,
    <= 3 * 2^-18 relative each -- the same 2e-4 bound, which the TF32 rounding of the reference's
    own GPU run would not meet at these K)."""
    from transplat_amd import kernels as K

    x1 = seeded((m, k1), 31)
    x2 = seeded((m, k2), 32) if k2 else None
    w = seeded((n, k1 + k2), 33) / math.sqrt(k1 + k2)
    b = seeded((n,), 34) if bias else None
    lnp = (seeded((n,), 35) * 0.1 + 1.0, seeded((n,), 36) * 0.1, 1e-5) if ln else None
    r = seeded((m, n), 37) if res else None
    ref = E.fused_linear(x1, w, x2=x2, bias=b, gelu=gelu, ln=lnp, residual=r, split=split, gelu_in=gin)
    d = lambda t: t.to(device) if t is not None else None
    with K.dense_precision(dense):
        out = K.fused_linear(d(x1), d(w), x2=d(x2), bias=d(b), gelu=gelu,
                             ln=(d(lnp[0]), d(lnp[1]), lnp[2]) if ln else None, residual=d(r), split=split,
                             gelu_in=gin)
    if split:
        assert len(out) == n // 128 and all(o.is_contiguous() and o.shape == (m, 128) for o in out)
        out, ref = torch.cat(out, -1), torch.cat(ref, -1)
    err = (out.cpu() - ref).abs().max().item()
    assert err < 2e-4 * max(1.0, ref.abs().max().item()), err


@pytest.mark.gpu
@pytest.mark.parametrize("hw,m,shift,b,res,kvs", [(64, 1, True, 2, True, 0), (64, 1, False, 2, False, 0),
                                                  (64, 2, True, 3, True, 0), (32, 1, True, 2, False, 0),
                                                  (64, 1, True, 8, True, 0), (64, 1, True, 2, True, 1),
                                                  (64, 1, False, 4, False, 2), (64, 1, True, 8, False, 4),
                                                  (64, 1, True, 1, True, 0),
                                                  pytest.param(WIDE, 1, True, 1, True, 0, id="32x96-1-True-1-True-0")])
@pytest.mark.parametrize("dense", ["fp32", "bf16x3"])
def test_attention_merge_kernel(device, monkeypatch, hw, m, shift, b, res, kvs, dense):
    """Window attention + merge Linear + LayerNorm (+ residual) with the split-key combine folded
    into the merge kernel (tsplat_win_attn_partials_fwd + tsplat_linear_f32_attn_merge_fwd; key
    splits 4 / 8 here, b = 8 takes the unsplit path) vs the CPU restatement; the merge's products
    exact fp32 or bf16x3 (dense mode)."""
    from transplat_amd import _lib
    from transplat_amd import kernels as K

    h, w = _map_hw(hw)
    q = seeded((b, h * w, 128), 41)
    k = seeded((b, m, h * w, 128), 42) if m > 1 else seeded((b, h * w, 128), 42)
    v = seeded(k.shape, 43)
    wm = seeded((128, 128), 44) / math.sqrt(128)
    ln = (seeded((128,), 45) * 0.1 + 1.0, seeded((128,), 46) * 0.1, 1e-5)
    r = seeded((b, h * w, 128), 47) if res else None
    ks = int(_lib.load().tsplat_win_attn_split(b, h, w, m, 2))
    assert (ks > 1) == (b < 8)
    ref = E.attention_merge(q, k, v, h, w, 2, shift, wm, ln, residual=r, kv_shift=kvs)
    d = lambda t: t.to(device) if t is not None else None
    with K.dense_precision(dense):
        out = K.attention_merge(d(q), d(k), d(v), h, w, 2, shift, d(wm), (d(ln[0]), d(ln[1]), ln[2]),
                                residual=d(r), kv_shift=kvs)
    err = (out.cpu() - ref).abs().max().item()
    assert err < 1e-3, err


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 3, 4])
def test_small_inverse_kernel(device, d):
    """tsplat_small_inverse vs float64 torch.linalg.inv on camera-like matrices (rigid c2w with
    translation, normalised / pixel intrinsics) and random well-conditioned ones, incl. rows that
    need pivoting."""
    from transplat_amd import kernels as K

    g = torch.Generator().manual_seed(d)
    a = torch.randn((257, d, d), generator=g) + 3.0 * torch.eye(d)
    a[::7] = a[::7].flip(-2)  # zero-free but pivot-requiring row orders
    if d >= 3:
        k = torch.eye(d).repeat(16, 1, 1)
        k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2] = 250.0, 260.0, 128.0, 127.5
        a = torch.cat([a, k])
    ref = torch.linalg.inv(a.double())
    out = K.small_inverse(a.to(device)).cpu().double()
    rel = ((out - ref).abs().amax((-2, -1)) / ref.abs().amax((-2, -1))).max().item()
    assert rel < 1e-5, rel


@pytest.mark.gpu
@pytest.mark.parametrize("shape,act,res", [((2, 64, 128, 128), "relu", False), ((2, 96, 64, 64), "relu", True),
                                           ((2, 128, 64, 64), "none", False), ((1, 3, 7, 9), "relu", True)])
def test_instance_norm_kernel(device, shape, act, res):
    """InstanceNorm2d (+ ReLU, + the ResidualBlock's relu(x + .)) through the GroupNorm kernel with
    one group per channel vs torch's instance_norm on the CPU."""
    from transplat_amd import kernels as K

    x = seeded(shape, 51) * 2.0 + 0.5
    r = seeded(shape, 52) if res else None
    ref = torch.nn.functional.instance_norm(x, eps=1e-5)
    if act == "relu":
        ref = torch.relu(ref)
    if res:
        ref = torch.relu(r + ref)
    np.testing.assert_allclose(E.instance_norm(x, 1e-5, act, r).numpy(), ref.numpy(), atol=1e-5)
    out = K.instance_norm(x.to(device), 1e-5, act, r.to(device) if res else None).cpu()
    assert (out - ref).abs().max().item() < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,hw,act,res", [(163, 168, 64, "gelu", False), (168, 84, 64, "none", False),
                                                 (64, 64, 37, "relu", False), (64, 64, 36, "none", True)])
def test_conv_bias_act(device, cin, cout, hw, act, res):
    """Bias-free MIOpen convolution + tsplat_bias_act_fwd (bias, GELU / ReLU, skip add in one pass)
    vs the module chain on the CPU (37x37: odd plane size takes the module path)."""
    from transplat_amd import kernels as K

    torch.manual_seed(0)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1)
    x = seeded((2, cin, hw, hw), 61)
    r = seeded((2, cout, hw, hw), 62) if res else None
    ref = E.conv_bias_act(conv, x, act, r)
    out = K.conv_bias_act(conv.to(device), x.to(device), act, r.to(device) if res else None).cpu()
    assert (out - ref).abs().max().item() < 2e-3 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["16", "16x8", "32"])
@pytest.mark.parametrize("b,n,heads", [(2, 325, 12), (1, 37, 12), (3, 5, 2), (1, 1025, 4), (1, 1, 1), (1, 16, 2),
                                       (2, 32, 1), (2, 33, 1), (1, 64, 3)])
def test_mha_kernel(device, b, n, heads, form, monkeypatch):
    """DINOv2 multi-head attention (tsplat_mha_f32_fwd, straight from the qkv layout) vs torch SDPA
    math on the CPU, for each kernel form (TSPLAT_MHA: 16-query blocks with 4 or 8 waves, 32-query
    blocks); N = 325 is the 256x256 token count, N = 5 leaves waves without keys, N = 1 all but one;
    N = 16 and 32 are whole tiles (nothing masked), N = 33 is one key past a tile, N = 64 is 4 tiles
    over the 8 waves of form 16x8."""
    from transplat_amd import kernels as K

    monkeypatch.setenv("TSPLAT_MHA", form)

    qkv = seeded((b, n, 3 * heads * 64), 71) * 2.0
    ref = E.mha(qkv, heads, 64 ** -0.5)
    out = K.mha(qkv.to(device), heads, 64 ** -0.5).cpu()
    assert out.shape == (b, n, heads * 64)
    assert (out - ref).abs().max().item() < 5e-5  # fp32, different summation order over up to 1025 keys


@pytest.mark.gpu
@pytest.mark.parametrize("b,n", [(2, 325), (1, 5), (1, 33)])
def test_mha_bias_folded(device, b, n):
    """tsplat_mha_bias_f32_fwd (qkv without the projection bias + the bias vector: q bias on load,
    k bias dropped -- the softmax cancels it -- v bias on the output) vs the CPU restatement on
    qkv + bias, same tolerance as test_mha_kernel."""
    from transplat_amd import kernels as K

    heads = 12
    qkv = seeded((b, n, 3 * heads * 64), 72) * 2.0
    bias = seeded((3 * heads * 64,), 73) * 0.5
    ref = E.mha(qkv + bias, heads, 64 ** -0.5)
    out = K.mha(qkv.to(device), heads, 64 ** -0.5, bias=bias.to(device)).cpu()
    assert (out - ref).abs().max().item() < 5e-5


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("b,n,heads", [(2, 325, 12), (16, 325, 12), (1, 37, 12), (3, 5, 2), (1, 1025, 4), (1, 1, 1),
                                       (1, 16, 2), (2, 32, 1), (2, 33, 1), (1, 64, 3)])
def test_mha_x3_kernel(device, b, n, heads, bias):
    """DINOv2 attention in split-bf16 precision (tsplat_mha_x3_fwd: qkv + bias split once into hi / lo
    bf16, QK^T and PV as hi*hi + hi*lo + lo*hi on bf16 MFMA, fp32 softmax) vs the float64 SDPA
    restatement on qkv + bias. Bound (written here): 1e-4 of max |O| -- the three-term split's
    ~1e-5 per product accumulated over the keys; TF32 operands would give ~1e-3."""
    from transplat_amd import kernels as K

    qkv = seeded((b, n, 3 * heads * 64), 74) * 2.0
    bv = seeded((3 * heads * 64,), 75) * 0.5 if bias else None
    full = qkv + bv if bias else qkv
    ref = E.mha(full.double(), heads, 64 ** -0.5)
    out = K.mha(qkv.to(device), heads, 64 ** -0.5, bias=bv.to(device) if bias else None, precision="bf16x3")
    assert out.shape == (b, n, heads * 64) and out.dtype == torch.float32
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"mha x3 b={b} n={n} heads={heads} bias={bias}: rel err {err:.2e}")
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim,with_y,with_ls", [(650, 768, True, True), (650, 768, False, False),
                                                     (7, 256, True, False), (33, 1024, True, True)])
def test_residual_ln_kernel(device, rows, dim, with_y, with_ls):
    """DINOv2 pre-norm residual step (x + ls * y, LayerNorm) in one launch vs the CPU restatement."""
    from transplat_amd import kernels as K

    norm = torch.nn.LayerNorm(dim, eps=1e-6)
    with torch.no_grad():
        norm.weight.copy_(seeded((dim,), 81) * 0.1 + 1.0)
        norm.bias.copy_(seeded((dim,), 82) * 0.1)
    x, y = seeded((rows, dim), 83) * 3.0, seeded((rows, dim), 84) if with_y else None
    ls = seeded((dim,), 85) if with_ls else None
    rx, rn = E.residual_ln(x, y, ls, norm)
    d = lambda t: t.to(device) if t is not None else None
    ox, on = K.residual_ln(d(x), d(y), d(ls), norm.to(device))
    assert (ox.cpu() - rx).abs().max().item() < 1e-5
    assert (on.cpu() - rn).abs().max().item() < 2e-5
    # bf16 form (bf16 dense mode): bf16 sub-layer output in, fp32 residual stream, bf16 LayerNorm
    # out = the fp32 result rounded once
    yb = y.bfloat16() if with_y else None
    rxb, rnb = E.residual_ln(x, yb.float() if with_y else None, ls, norm.cpu())
    oxb, onb = K.residual_ln(d(x), d(yb), d(ls), norm.to(device), bf16_out=True)
    assert onb.dtype == torch.bfloat16 and oxb.dtype == torch.float32
    assert (oxb.cpu() - rxb).abs().max().item() < 1e-5
    assert (onb.float().cpu() - rnb).abs().max().item() < 8e-3 * max(1.0, rnb.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("k,relu_in", [(128, False), (256, True)])
def test_fused_linear_post_norm(device, k, relu_in):
    """UV encoder post-norm form LN(x W^T + b + identity) (+ ReLU on the FFN hidden input)."""
    from transplat_amd import kernels as K

    m = 2 * 4096
    x = seeded((m, k), 91)
    w = seeded((128, k), 92) / math.sqrt(k)
    b = seeded((128,), 93)
    r = seeded((m, 128), 94)
    lnp = (seeded((128,), 95) * 0.1 + 1.0, seeded((128,), 96) * 0.1, 1e-5)
    ref = E.fused_linear(x, w, bias=b, ln=lnp, residual=r, relu_in=relu_in, res_pre_ln=True)
    d = lambda t: t.to(device)
    out = K.fused_linear(d(x), d(w), bias=d(b), ln=(d(lnp[0]), d(lnp[1]), lnp[2]), residual=d(r), relu_in=relu_in,
                         res_pre_ln=True).cpu()
    assert (out - ref).abs().max().item() < 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,h,w", [(2, 128, 64, 64), (1, 37, 9, 11), (3, 256, 8, 8)])
def test_depth_softmax_kernel(device, n, d, h, w):
    """Depth-candidate softmax head (expected disparity + max pdf) vs the CPU restatement."""
    from transplat_amd import kernels as K

    logits = seeded((n, d, h, w), 97) * 4.0
    disp = torch.linspace(0.01, 1.0, d).repeat(n, 1).reshape(n, d, 1, 1)
    rc, rm = E.depth_softmax(logits, disp)
    oc, om = K.depth_softmax(logits.to(device), disp.to(device))
    # 2e-6 on O(1) values: the kernel merges 8 depth slices' sums with an exp(m_slice - M) rescale
    assert (oc.cpu() - rc).abs().max().item() < 2e-6 and (om.cpu() - rm).abs().max().item() < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("shape,scale,act,bias", [((2, 128, 64, 64), 4, "gelu", True), ((1, 3, 5, 7), 4, "none", False),
                                                   ((2, 8, 16, 16), 2, "relu", True)])
def test_upsample_bilinear_act_kernel(device, shape, scale, act, bias):
    """Depth predictor upsampler tail (bias -> bilinear align_corners -> GELU) vs the oracle."""
    from transplat_amd import kernels as K

    x = seeded(shape, 71)
    b = seeded((shape[1],), 72) if bias else None
    ref = E.upsample_bilinear_act(x, scale, b, act)
    out = K.upsample_bilinear_act(x.to(device), scale, b.to(device) if b is not None else None, act).cpu()
    # rounding-level: the source coordinate o (in - 1) / (out - 1) is an fp32 value up to 63 (ulp
    # 3.8e-6), so a one-ulp different rounding moves an interpolation weight by ~4e-6; the bias is
    # added after the interpolation (exact in real arithmetic)
    assert (out - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("vb,heads,views,t", [(2, 4, 2, 256), (2, 1, 2, 256), (3, 2, 1, 100), (4, 1, 2, 37),
                                                  (6, 2, 3, 40), (6, 1, 3, 37), (1, 1, 1, 1), (2, 1, 2, 16)])
def test_qkv_attention_cf_kernel(device, vb, heads, views, t):
    """U-Net legacy QKV attention (head dim 32, views folded into the tokens) vs the oracle; the
    vb = 6 cases fold 3 views of 2 scenes (row view * 2 + scene); T = 1 is one key, T = 2 x 16 exactly
    one tile (seven waves without keys)."""
    from transplat_amd import kernels as K

    qkv = seeded((vb, 3 * heads * 32, t), 81) * 2.0
    ref = E.qkv_attention_cf(qkv, heads, views)
    out = K.qkv_attention_cf(qkv.to(device), heads, views).cpu()
    assert (out - ref).abs().max().item() < 5e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape,size", [((2, 128, 9, 9), (18, 18)), ((2, 128, 72, 72), (144, 144)),
                                        ((2, 64, 144, 144), (252, 252)), ((1, 4, 5, 3), (7, 11))])
def test_resize_bilinear_nhwc_kernel(device, shape, size):
    """DPT channels-last bilinear resizes (align_corners) vs the oracle (torch interpolate on CPU)."""
    from transplat_amd import kernels as K

    x = seeded(shape, 91)
    ref = E.resize_bilinear_nhwc(x, size)
    out = K.resize_bilinear_nhwc(x.to(device).contiguous(memory_format=torch.channels_last), size)
    assert out.is_contiguous(memory_format=torch.channels_last)
    # fp32 source-coordinate rounding (see the upsample test): 1e-5 of the map's scale
    assert (out.cpu() - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("y_bf16,out_bf16,res", [(False, False, False), (False, False, True), (True, False, True),
                                                 (True, True, False), (False, True, False)])
def test_layer_norm128_kernel(device, y_bf16, out_bf16, res):
    """[residual +] LayerNorm over 128-wide rows (the bf16-mode MVT / UV norms) vs torch on CPU, on the
    same (bf16-rounded where bf16) inputs; rows not a multiple of the 8 rows per workgroup."""
    from transplat_amd import kernels as K

    norm = torch.nn.LayerNorm(128)
    with torch.no_grad():
        norm.weight.copy_(seeded((128,), 86) * 0.1 + 1.0)
        norm.bias.copy_(seeded((128,), 87) * 0.1)
    y = seeded((3, 1001, 128), 88) * 2.0 + 0.5
    if y_bf16:
        y = y.bfloat16()
    r = seeded((3, 1001, 128), 89) if res else None
    with torch.no_grad():
        ref = norm(y.float()) + (r if res else 0.0)
    out = K.layer_norm128(y.to(device), norm.to(device), residual=r.to(device) if res else None,
                          out_dtype=torch.bfloat16 if out_bf16 else torch.float32)
    assert out.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
    tol = 8e-3 * ref.abs().max().item() if out_bf16 else 2e-5 * max(1.0, ref.abs().max().item())
    assert (out.float().cpu() - ref).abs().max().item() < tol


def test_oracle_bilinear_zero_grid_sample_matches_corners():
    """The oracle's sampler (F.grid_sample, the reference CPU path's operator) against the explicit
    four-corner zero-padded bilinear form, including out-of-map and edge samples."""
    g = torch.Generator().manual_seed(5)
    img = torch.randn(16, 20, 8, generator=g)
    x = torch.rand(300, 5, generator=g) * 26 - 3
    y = torch.rand(300, 5, generator=g) * 22 - 3
    a, b = E.bilinear_zero(img, x, y), E.bilinear_zero_corners(img, x, y)
    assert a.shape == b.shape == (300, 5, 8)
    # coordinates are rounded differently (grid_sample unnormalises (g + 1) W / 2 - 1 / 2): a few ulps
    # of a coordinate times the map's slope
    assert (a - b).abs().max().item() < 2e-5
