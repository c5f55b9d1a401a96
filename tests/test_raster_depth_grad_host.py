"""Fused colour + depth + alpha backward, the parts that need no GPU: the composed float64 yardstick
(tests/raster_depth_grad_ref.py) against the literal oracle's depth render and against finite differences, and
the host-side contract of tsplat_raster_depth_bwd (header, exports, signature table, argument checks before any
launch, the decoder flags, no CPU path)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import raster_depth_grad_ref as dref
import raster_grad_cases as cases
import raster_grad_ref
import test_raster_depth as depth_scenes
from test_raster_grad_host import _small_case
from transplat_amd import _lib
from transplat_amd.model.decoder.decoder_splatting_hip import DecoderSplattingHIPCfg, depth_fake_color
from transplat_amd.model.decoder.hip_splatting import RasterCameras

ROOT = Path(__file__).resolve().parent.parent
MODES = depth_scenes.MODES


# ------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name,mode", [("B", m) for m in MODES] + [("D", "depth")])
def test_composed_depth_and_alpha_match_literal_oracle(name, mode):
    """Scenes B and D are test_raster_depth.py's, whose literal-oracle depth and alpha renders are the reference:
    unflagged pixels of the rendered views within that file's forward bar (ATOL x scale)."""
    ref = dref.reference(name, mode)
    dref.check_conditions(ref)
    rendered = ref["rendered"]
    for what, got in (("depth", ref["depth"]), ("alpha", ref["alpha"])):
        img, _, pflag, _ = depth_scenes.reference(name, mode if what == "depth" else "alpha")
        want = torch.from_numpy(np.array(img)).double()
        clear = ~ref["flagged"] & torch.from_numpy(np.array(pflag) == 0)
        scale = max(float(want[rendered].abs().max()), 1.0)
        linf = float((got - want).abs()[clear].max())
        print(f"{name} {mode} {what}: composed vs oracle L-inf {linf:.3e} (scale {scale:.3g}) on {int(clear.sum())} "
              f"unflagged pixels; flagged {ref['flagged_fraction']:.3%}; visible {ref['visible']}, clamped "
              f"{ref['clamped']}, depth kinks {ref['depth_kinks']}")
        assert int(clear.sum()) > 0 and float(want[clear].abs().max()) > 0
        assert linf <= depth_scenes.ATOL * scale
    for g in ref["grads"]:
        assert torch.isfinite(g).all()
    assert float(ref["grads"][0].abs().max()) > 0


def test_scene_conditions_hold_for_every_gpu_case():
    """The conditions the GPU tests rely on: flagged share, no kink, no visible Gaussian within 1e-5 of the depth
    value's clamp; the clamp and log-branch scenes do what their tests need."""
    for name, mode in [("tiny", m) for m in MODES] + [("tiny_s1", "depth"), ("C16", "depth")]:
        dref.check_conditions(dref.reference(name, mode))
    ref = dref.reference("B", "relative_disparity", "clamp")
    dref.check_conditions(ref)
    print(f"clamp: {ref['clamped']} of {ref['visible']} visible Gaussians clamped")
    assert ref["clamped"] >= 0.05 * ref["visible"]
    ref = dref.reference("B", "log", "swap")
    dref.check_conditions(ref)
    print(f"log, planes swapped: {ref['log_inside']} of {ref['visible']} visible Gaussians strictly inside")
    assert 0 < ref["log_inside"] < ref["visible"]
    assert dref.reference("B", "log")["log_inside"] == 0


@pytest.mark.parametrize("mode", MODES)
def test_gradcheck_smooth_core_depth_and_alpha(mode):
    """torch.autograd.gradcheck of the composed depth and alpha renders on an 8x8 image, decisions frozen."""
    (means, cov, sh, op), cams = _small_case()
    dark = RasterCameras(cams.viewmat, cams.projmat, cams.campos, cams.tanfov, torch.zeros_like(cams.bg), cams.scale)
    base = raster_grad_ref.render(means, cov, sh, op, cams, (8, 8), 1, 3)
    assert base["kinks"] == 0 and not base["ambiguous"].any()
    # the camera of _small_case is the identity at scale 1.5: unscaled c2w = identity; "log" with the planes
    # swapped so that its pass branch (far < z < near) is the one checked
    ext = torch.eye(4, dtype=torch.float64)[None]
    near, far = torch.tensor([0.5], dtype=torch.float64), torch.tensor([50.0], dtype=torch.float64)
    if mode == "log":
        near, far = far, near
    one = torch.full((1, means.shape[1], 3, 1), 0.5 / raster_grad_ref.C0, dtype=torch.float64)

    def f(m, c, o):
        fake = depth_fake_color(ext, m, near, far, mode)  # [1, G]
        kw = dict(frozen=base["decisions"], create_graph=True)
        depth = raster_grad_ref.render(m, c, fake[:, :, None, None].expand(-1, -1, 3, 1), o, dark, (8, 8), 1, 0, **kw)
        alpha = raster_grad_ref.render(m, c, one, o, dark, (8, 8), 1, 0, **kw)
        assert depth["kinks"] == 0
        return depth["color"].mean(dim=1), alpha["color"].mean(dim=1)

    leaves = [t.clone().requires_grad_() for t in (means, cov, op)]
    d, a = (t.detach() for t in f(*leaves))
    assert float(d.max()) > 0.05 and 0.05 < float(a.max()) <= 1.0
    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


# ------------------------------------------------------------------------------ the entry point
def test_header_declares_and_library_exports_depth_backward():
    header = (ROOT / "include" / "transplat_hip.h").read_text()
    m = re.search(r"\bint\s+tsplat_raster_depth_bwd\s*\(([^;]*)\)\s*;", header)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    lib = _lib.load()
    assert hasattr(lib, "tsplat_raster_depth_bwd") and "tsplat_raster_depth_bwd" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["tsplat_raster_depth_bwd"]
    assert res is ctypes.c_int and len(args) == len(params) == len(BWD_NAMES) + 1
    for p, a in zip(params, args):  # int32_t <-> c_int32, every pointer <-> a pointer type
        assert ("*" in p) == (a is not ctypes.c_int32), p
    assert params[1 + BWD_NAMES.index("mode")].startswith("int32_t")
    # the same gradient records as tsplat_raster_bwd: the workspace size is unchanged
    assert lib.tsplat_raster_bwd_workspace_bytes(1000, 3) == 1000 * 3 * 64
    assert _lib.PROF_IDS["raster_bwd_render"] == 17 and _lib.PROF_IDS["raster_bwd"] == 19


BWD_NAMES = ["means", "cov", "shs", "opacity", "viewmat", "projmat", "campos", "tanfov", "bg", "scene_scale", "near", "far",
             "mode", "out_color", "out_depth", "out_alpha", "grad_color", "grad_depth", "grad_alpha", "radii",
             "fwd_workspace", "bwd_workspace", "grad_means", "grad_cov", "grad_shs", "grad_opacity", "stream"]
BWD_OUTPUTS = ["grad_means", "grad_cov", "grad_shs", "grad_opacity"]
PAIRS = [("grad_color", "out_color"), ("grad_depth", "out_depth"), ("grad_alpha", "out_alpha")]


def _bwd_args(ptrs, desc=None, **over):
    vals = {n: ptrs.get(n, ptrs.get("*")) for n in BWD_NAMES}
    vals["stream"], vals["mode"] = None, 0
    vals.update(over)
    desc = desc or _lib.RasterDesc(1, 1, 1, 16, 16, 1, 0, 16)
    return [ctypes.byref(desc)] + [vals[n] for n in BWD_NAMES]


def test_depth_bwd_einval_before_any_launch():
    """Every argument rule of tsplat_raster_depth_bwd is checked before the first launch, so host pointers are
    enough (a launch would fail, with another status, on a host without a device)."""
    lib = _lib.load()
    host = ctypes.create_string_buffer(4096)
    p = {"*": ctypes.addressof(host)}
    call = lambda *a, **k: lib.tsplat_raster_depth_bwd(*_bwd_args(p, *a, **k))
    einval = -1
    assert call(grad_color=None, grad_depth=None, grad_alpha=None) == einval  # no gradient given
    assert call(**{n: None for pair in PAIRS for n in pair}) == einval
    for grad, out in PAIRS:  # a gradient without its saved output, alone or beside the others
        assert call(**{out: None}) == einval, out
        others = {n: None for pair in PAIRS if pair[0] != grad for n in pair}
        assert call(**{out: None}, **others) == einval, out
    for missing in ({"near": None}, {"far": None}, {"near": None, "far": None}):  # grad_depth needs both planes
        assert call(**missing) == einval
        assert call(**missing, grad_color=None, out_color=None, grad_alpha=None, out_alpha=None) == einval
    for mode in (-1, 4, 1 << 20):
        assert call(mode=mode) == einval
        assert call(mode=mode, grad_depth=None, out_depth=None) == einval  # out of range even without a depth gradient
    assert call(**{n: None for n in BWD_OUTPUTS}) == einval  # no gradient asked for
    # what tsplat_raster_bwd rejects
    for name in ("means", "cov", "shs", "opacity", "viewmat", "projmat", "campos", "tanfov", "bg", "scene_scale", "radii",
                 "fwd_workspace", "bwd_workspace"):
        assert call(**{name: None}) == einval, name
        assert call(**{name: None}, grad_color=None, out_color=None) == einval, name
    for bad in (_lib.RasterDesc(0, 1, 1, 16, 16, 1, 0, 16), _lib.RasterDesc(1, 3, 2, 16, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 16, 1, 1, 16), _lib.RasterDesc(1, 1, 1, 16, 16, 1, 0, 0),
                _lib.RasterDesc(1, 1, 1, 16, 16, 26, 0, 16), _lib.RasterDesc(1, 33, 33, 16, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 1 << 20, 1, 0, 16), _lib.RasterDesc(1, 1, 1, 0, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 16, 1, 5, 16)):
        assert call(bad) == einval
        for grad, out in PAIRS:  # also with a single gradient given
            assert call(bad, **{n: None for pair in PAIRS if pair[0] != grad for n in pair}) == einval
    assert lib.tsplat_raster_depth_bwd(None, *_bwd_args(p)[1:]) == einval


# ------------------------------------------------------------------------------ Python side
def test_decoder_depth_flag_defaults_to_off_and_needs_differentiable():
    assert DecoderSplattingHIPCfg().differentiable_depth is False
    assert DecoderSplattingHIPCfg(differentiable=True).differentiable_depth is False
    assert DecoderSplattingHIPCfg(differentiable=True, differentiable_depth=True).differentiable_depth is True
    with pytest.raises(ValueError, match="differentiable=True"):
        DecoderSplattingHIPCfg(differentiable_depth=True)


def test_rasterize_with_depth_differentiable_needs_device_tensors():
    """No CPU path: host tensors raise as rasterize() does, with or without requires_grad."""
    from transplat_amd.model.decoder.hip_splatting import rasterize, rasterize_with_depth_differentiable

    c = cases.case("tiny")
    g = c["g"]
    cams = cases.cameras("tiny")
    args = lambda m: (m, g["covariances"], g["harmonics"], g["opacities"], cams, c["hw"], c["vps"])
    with pytest.raises(RuntimeError, match="device tensors") as plain:
        rasterize(*args(g["means"]))
    for m in (g["means"], g["means"].clone().requires_grad_()):
        with pytest.raises(RuntimeError, match="device tensors") as diff:
            rasterize_with_depth_differentiable(*args(m), near=c["near"], far=c["far"], depth_mode="depth", alpha=True)
        assert str(diff.value) == str(plain.value)
    with pytest.raises(ValueError, match="depth_mode"):
        rasterize_with_depth_differentiable(*args(g["means"]), near=c["near"], far=c["far"], depth_mode="metres")
    with pytest.raises(ValueError, match="near and far"):
        rasterize_with_depth_differentiable(*args(g["means"]), depth_mode="depth")
