"""Rasterizer backward, the parts that need no GPU: the float64 yardstick (tests/raster_grad_ref.py) against
the literal oracle and against finite differences, and the host-side contract of the new entry point
(header, exports, argument checks before any launch, the decoder flag's default, no CPU path)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import raster_grad_cases as cases
import raster_grad_ref
from transplat_amd import _lib
from transplat_amd.model.decoder.decoder_splatting_hip import DecoderSplattingHIPCfg
from transplat_amd.model.decoder.hip_splatting import RasterCameras

ROOT = Path(__file__).resolve().parent.parent
FWD_ATOL = 1e-4  # the forward's own bar against the literal oracle, x scale = max(|ref|.max(), 1)


# ------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_colour_matches_literal_oracle(name):
    """Unflagged pixels within the forward's bar; the conditions on the scenes hold (at most 1 % of the pixels
    flagged, no Gaussian-level kink); radii agree wherever the oracle rendered."""
    ref = cases.reference(name)
    rendered = ref["rendered"]
    clear = ~ref["flagged"]
    want = ref["oracle_color"].double()
    scale = max(float(want[rendered].abs().max()), 1.0)
    err = (ref["color"] - want).abs().amax(dim=1)
    linf = float(err[clear].max())
    same_radii = float((ref["radii"][rendered] == ref["oracle_radii"][rendered]).double().mean())
    print(f"{name}: restatement vs oracle L-inf {linf:.3e} (scale {scale:.3g}) on {int(clear.sum())} unflagged pixels; "
          f"flagged {ref['flagged_fraction']:.3%}; kinks {ref['kinks']}; radii equal {same_radii:.4%}")
    assert int(clear.sum()) > 0
    assert linf <= FWD_ATOL * scale
    assert ref["flagged_fraction"] <= cases.MAX_FLAGGED
    assert ref["kinks"] == 0
    assert same_radii >= 1 - 1e-3
    for g in ref["grads"]:
        assert torch.isfinite(g).all()
    assert float(ref["grads"][0].abs().max()) > 0


def _small_case():
    """6 Gaussians in front of an identity camera, one 8x8 image."""
    gen = torch.Generator().manual_seed(3)
    n = 6
    means = torch.zeros((1, n, 3), dtype=torch.float64)
    means[0, :, :2] = (torch.rand((n, 2), generator=gen, dtype=torch.float64) - 0.5) * 0.6
    means[0, :, 2] = 2.0 + torch.rand(n, generator=gen, dtype=torch.float64) * 2.0
    a = torch.randn((n, 3, 3), generator=gen, dtype=torch.float64) * 0.15
    cov = (a @ a.transpose(1, 2) + 0.01 * torch.eye(3, dtype=torch.float64))[None]
    sh = torch.randn((1, n, 3, 16), generator=gen, dtype=torch.float64) * 0.3
    op = 0.2 + 0.6 * torch.rand((1, n), generator=gen, dtype=torch.float64)
    eye = torch.eye(4, dtype=torch.float64).reshape(1, 16)
    proj = torch.tensor([[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 1.01, -1.01], [0, 0, 1.0, 0]], dtype=torch.float64)
    cams = RasterCameras(viewmat=eye, projmat=proj.T.reshape(1, 16).contiguous(), campos=torch.zeros((1, 3), dtype=torch.float64),
                         tanfov=torch.full((1, 2), 0.5, dtype=torch.float64), bg=torch.full((1, 3), 0.3, dtype=torch.float64),
                         scale=torch.tensor([[1.5, 2.25]], dtype=torch.float64))
    return (means, cov, sh, op), cams


def test_gradcheck_smooth_core():
    """torch.autograd.gradcheck of the restatement with the decisions of the unperturbed inputs frozen."""
    inputs, cams = _small_case()
    base = raster_grad_ref.render(*inputs, cams, (8, 8), 1, 3)
    assert base["kinks"] == 0 and not base["ambiguous"].any()
    assert float((base["color"] - 0.3).abs().max()) > 0.05  # the Gaussians are in the picture
    leaves = [t.clone().requires_grad_() for t in inputs]

    def f(m, c, s, o):
        # symmetrise nothing: the six upper-triangle entries are the function's arguments
        return raster_grad_ref.render(m, c, s, o, cams, (8, 8), 1, 3, frozen=base["decisions"], create_graph=True)["color"]

    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)
    # the lower triangle of the covariances is not read
    (gc,) = torch.autograd.grad(f(*leaves).square().sum(), leaves[1])
    assert float(gc[0, :, 1, 0].abs().max()) == 0 and float(gc[0, :, 2, 0].abs().max()) == 0
    assert float(gc[0, :, 2, 1].abs().max()) == 0 and float(gc[0, :, 0, 1].abs().max()) > 0


# ------------------------------------------------------------------------------ the entry point
def test_header_declares_and_library_exports_backward():
    header = (ROOT / "include" / "transplat_hip.h").read_text()
    assert re.search(r"\bsize_t\s+tsplat_raster_bwd_workspace_bytes\s*\(", header)
    assert re.search(r"\bint\s+tsplat_raster_bwd\s*\(", header)
    lib = _lib.load()
    assert hasattr(lib, "tsplat_raster_bwd") and hasattr(lib, "tsplat_raster_bwd_workspace_bytes")
    assert "tsplat_raster_bwd" in _lib.SIGNATURES and "tsplat_raster_bwd_workspace_bytes" in _lib.SIGNATURES
    # one 64-byte record per (view, Gaussian), 256-byte aligned
    assert lib.tsplat_raster_bwd_workspace_bytes(1000, 3) == 1000 * 3 * 64
    assert lib.tsplat_raster_bwd_workspace_bytes(1, 1) == 256


BWD_NAMES = ["means", "cov", "shs", "opacity", "viewmat", "projmat", "campos", "tanfov", "bg", "scene_scale", "out_color",
             "grad_color", "radii", "fwd_workspace", "bwd_workspace", "grad_means", "grad_cov", "grad_shs", "grad_opacity",
             "stream"]
BWD_OUTPUTS = ["grad_means", "grad_cov", "grad_shs", "grad_opacity"]


def _bwd_args(ptrs, desc=None, **over):
    vals = {n: ptrs.get(n, ptrs.get("*")) for n in BWD_NAMES}
    vals["stream"] = None
    vals.update(over)
    desc = desc or _lib.RasterDesc(1, 1, 1, 16, 16, 1, 0, 16)
    return [ctypes.byref(desc)] + [vals[n] for n in BWD_NAMES]


def test_bwd_einval_before_any_launch():
    """Every argument rule of tsplat_raster_bwd is checked before the first launch, so host pointers are enough
    (a launch would fail, with another status, on a host without a device)."""
    lib = _lib.load()
    host = ctypes.create_string_buffer(4096)
    p = {"*": ctypes.addressof(host)}
    call = lambda *a, **k: lib.tsplat_raster_bwd(*_bwd_args(p, *a, **k))
    einval = -1
    assert call(**{n: None for n in BWD_OUTPUTS}) == einval  # no gradient asked for
    for name in BWD_NAMES:
        if name not in BWD_OUTPUTS and name != "stream":
            assert call(**{name: None}) == einval, name
    # the descriptor rules of tsplat_raster_fwd
    for bad in (_lib.RasterDesc(0, 1, 1, 16, 16, 1, 0, 16), _lib.RasterDesc(1, 3, 2, 16, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 16, 1, 1, 16), _lib.RasterDesc(1, 1, 1, 16, 16, 1, 0, 0),
                _lib.RasterDesc(1, 1, 1, 16, 16, 26, 0, 16), _lib.RasterDesc(1, 33, 33, 16, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 1 << 20, 1, 0, 16), _lib.RasterDesc(1, 1, 1, 0, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 16, 1, 5, 16)):
        assert call(bad) == einval
        for only in BWD_OUTPUTS:  # also with a single output wanted
            assert call(bad, **{n: None for n in BWD_OUTPUTS if n != only}) == einval
    assert lib.tsplat_raster_bwd(None, *_bwd_args(p)[1:]) == einval


# ------------------------------------------------------------------------------ Python side
def test_decoder_flag_defaults_to_off():
    assert DecoderSplattingHIPCfg().differentiable is False


def test_rasterize_differentiable_needs_device_tensors():
    """No CPU path: host tensors raise as rasterize() does, with or without requires_grad."""
    from transplat_amd.model.decoder.hip_splatting import rasterize, rasterize_differentiable

    c = cases.case("tiny")
    g = c["g"]
    cams = cases.cameras("tiny")
    args = lambda m: (m, g["covariances"], g["harmonics"], g["opacities"], cams, c["hw"], c["vps"])
    with pytest.raises(RuntimeError, match="device tensors") as plain:
        rasterize(*args(g["means"]))
    for m in (g["means"], g["means"].clone().requires_grad_()):
        with pytest.raises(RuntimeError, match="device tensors") as diff:
            rasterize_differentiable(*args(m))
        assert str(diff.value) == str(plain.value)
