"""The Depth-Anything glue kernels (csrc/daglue.hip, the broadcast residual of
tsplat_residual_ln_slabs_bcast_fwd) against the launches they replace: bit for bit where the arithmetic
is the same."""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from canonical import seeded  # noqa: E402


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,gh,gw", [(32, 32, 2, 2), (46, 32, 3, 2)])
def test_da_patches_equal_torch_sequence(device, h, w, gh, gw):
    """tsplat_da_patches_fwd == normalise, channel reorder (2, 0, 1), interpolate_bilinear_ac to
    (14 gh, 14 gw), unfold -- torch.equal; the class-token rows exactly zero."""
    from transplat_amd import kernels as K

    p = 14
    images = seeded((1, 2, 3, h, w), 301, kind="rand").to(device)
    mean = torch.tensor([0.485, 0.456, 0.406], device=device)
    std = torch.tensor([0.229, 0.224, 0.225], device=device)
    x = (images - mean.reshape(1, 1, 3, 1, 1)) / std.reshape(1, 1, 3, 1, 1)
    x = torch.cat((x[:, :, 2:3], x[:, :, 0:2]), dim=2).reshape(2, 3, h, w)
    x = K.interpolate_bilinear_ac(x, (gh * p, gw * p))
    ref = x.reshape(2, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(2, gh * gw, 3 * p * p)
    out = K.da_patches(images, mean, std, (gh, gw), p)
    assert out.shape == (2 * (1 + gh * gw), 3 * p * p)
    out = out.view(2, 1 + gh * gw, 3 * p * p)
    assert torch.equal(out[:, 0], torch.zeros_like(out[:, 0]))
    assert torch.equal(out[:, 1:], ref)
    assert torch.equal(K.da_patches(images, mean, std, (gh, gw), p).view_as(out), out)


@pytest.mark.gpu
def test_depth_norm_equals_torch_sequence(device):
    """tsplat_depth_norm_fwd == ReLU, resize to (24, 24), per-view aminmax / amin / amax, (d - min) /
    (max - min) as separate launches -- torch.equal; repeated launches bit-identical (576 pixels per
    view: three workgroups' partials, the last partly filled)."""
    from transplat_amd import kernels as K

    b, v, h, w = 1, 2, 24, 24
    x = (seeded((2, 1, 20, 20), 321) + 0.5).to(device)
    assert (x < 0).any() and (x > 0).any()
    d = F.relu(F.relu(x)).squeeze(1)
    d = K.interpolate_bilinear_ac(d[None].float().contiguous(), (h, w))
    d = d.view(b, v, 1, h, w).flatten(2)
    lo, hi = torch.aminmax(d.view(b, v, h, w), dim=-1)
    d_min, d_max = lo.amin(dim=-1, keepdim=True), hi.amax(dim=-1, keepdim=True)
    ref = ((d - d_min) / (d_max - d_min)).reshape(b, v, 1, h, w)
    out = K.depth_norm(x.reshape(2, 20, 20), (h, w)).view(b, v, 1, h, w)
    assert torch.equal(out, ref)
    assert out.min().item() == 0.0 and out.max().item() == 1.0
    for _ in range(3):
        assert torch.equal(K.depth_norm(x.reshape(2, 20, 20), (h, w)).view_as(out), out)


@pytest.mark.gpu
def test_residual_ln_broadcast_residual(device):
    """residual_ln with one [R, C] residual for every image (tsplat_residual_ln_slabs_bcast_fwd; two
    images, R = 7, C = 256, three slabs) against the materialised sum and F.layer_norm in float64, at
    test_residual_ln_kernel's bounds (1e-5 on x, 2e-5 on the normalised rows)."""
    from transplat_amd import kernels as K

    base = seeded((1, 7, 256), 331) * 3.0
    slabs = seeded((3, 2, 7, 256), 332)
    norm = torch.nn.LayerNorm(256, eps=1e-6)
    with torch.no_grad():
        norm.weight.copy_(seeded((256,), 333) * 0.1 + 1.0)
        norm.bias.copy_(seeded((256,), 334) * 0.1)
    rx = base.double() + slabs.double().sum(0)
    rn = F.layer_norm(rx, (256,), norm.weight.double(), norm.bias.double(), 1e-6)
    ox, on = K.residual_ln(base.to(device), slabs.to(device), None, norm.to(device))
    assert ox.shape == (2, 7, 256) and on.shape == (2, 7, 256)
    ex, en = (ox.cpu().double() - rx).abs().max().item(), (on.cpu().double() - rn).abs().max().item()
    print(f"residual_ln broadcast: x err {ex:.2e}, LN err {en:.2e}")
    assert ex < 1e-5 and en < 2e-5
    # the same bits as the repeated residual through the plain slabs entry point
    px, pn = K.residual_ln(base.to(device).expand(2, 7, 256).contiguous(), slabs.to(device), None, norm)
    assert torch.equal(ox, px) and torch.equal(on, pn)

