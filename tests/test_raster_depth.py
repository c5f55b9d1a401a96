"""Depth and alpha as outputs of the one rasterizer pass (tsplat_raster_depth_fwd,
rasterize_with_depth, DecoderSplattingHIP(depth_mode=...), GraphedStep(depth_mode=...)).

Reference of every parity test: the literal oracle (oracle.raster.render_flagged) on the Gaussians
repeated per view (S = V, views_per_scene = 1) with harmonics = depth_fake_color(...) computed on the
CPU, degree 0, background 0, mean over the channels -- the reference's render_depth_cuda path. Bars:
the project's own for a depth render (tests/test_raster.py, test_hip_render_depth_vs_reference_inputs),
relative to scale = max(|ref|.max(), 1): L-inf <= 1e-4 scale on unflagged pixels, every pixel within
2e-2 scale, at most 1e-3 of the pixels above 1e-4 scale, at most 1 % of the pixels flagged, radii
identical except at most 1e-3 of them ambiguous.
"""
import ctypes
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import raster as oracle_raster
from transplat_amd import _lib
from transplat_amd import synthetic as S
from transplat_amd.model.decoder.decoder_splatting_hip import (DecoderSplattingHIP, DecoderSplattingHIPCfg,
                                                               depth_fake_color)
from transplat_amd.model.decoder.hip_splatting import prepare_cameras, rasterize
from transplat_amd.model.types import Gaussians

ATOL = 1e-4
FLAGGED_CAP = 2e-2
MAX_ABOVE = 1e-3
MAX_FLAGGED = 0.01
MAX_AMBIGUOUS_RADII = 1e-3
MODES = ["depth", "disparity", "relative_disparity", "log"]
DC_ONE = 0.5 / 0.28209479177387814  # degree-0 coefficient of colour 1


# ------------------------------------------------------------------------------------ scenes
def _flat_target(batch):
    t = batch["target"]
    b, v = t["near"].shape
    return (t["extrinsics"].reshape(b * v, 4, 4), t["intrinsics"].reshape(b * v, 3, 3), t["near"].reshape(-1),
            t["far"].reshape(-1), v)


def _identity_camera(near):
    return (torch.eye(4)[None], S.intrinsics(1), torch.full((1,), near), torch.full((1,), 100.0), 1)


@lru_cache(maxsize=None)
def scene(name):
    """(gaussians dict [S, G, ...], extrinsics [V, 4, 4], intrinsics [V, 3, 3], near [V], far [V], views per scene)"""
    if name == "A":  # two scenes x three views from un-repeated buffers, a partial tile row, s = 2
        hw = (40, 56)
        return (S.make_gaussians(2, image_shape=hw), *_flat_target(S.make_batch(2, image_shape=hw, near=0.5, far=50.0)), hw)
    if name == "B":  # near-plane culls; relative_disparity reaches the clamp at 0
        hw = (64, 64)
        return (S.make_gaussians(1, image_shape=hw, depth_range=(0.05, 3.0)), *_flat_target(S.make_batch(1, image_shape=hw)), hw)
    if name == "C":  # > 4096 instances in one tile: the in-global-memory walk (test_raster_long_tile_lists_global_sort_path)
        n = 9000
        gen = torch.Generator().manual_seed(5)
        means = torch.zeros((1, n, 3))
        means[0, :, 0] = (torch.rand(n, generator=gen) - 0.5) * 0.05
        means[0, :, 1] = (torch.rand(n, generator=gen) - 0.5) * 0.05
        means[0, :, 2] = 4.0 + torch.rand(n, generator=gen)
        cov = (torch.eye(3) * 1e-4).expand(1, n, 3, 3).clone()
        sh = torch.randn((1, n, 3, 16), generator=gen) * S.sh_mask(3)
        op = torch.rand((1, n), generator=gen) * 0.3
        g = {"means": means, "covariances": cov, "harmonics": sh, "opacities": op}
        return (g, *_identity_camera(2.0), (64, 64))
    if name == "D":  # 2,500 Gaussians on 64 distinct depths: the counting sort (test_raster_tile_sort_..., 'ties')
        n = 2500
        gen = torch.Generator().manual_seed(11)
        means = torch.zeros((1, n, 3))
        means[0, :, 0] = (torch.rand(n, generator=gen) - 0.5) * 0.3
        means[0, :, 1] = (torch.rand(n, generator=gen) - 0.5) * 0.3
        means[0, :, 2] = 3.0 + torch.randint(0, 64, (n,), generator=gen).float() * 0.05
        cov = (torch.eye(3) * 4e-4).expand(1, n, 3, 3).clone()
        sh = torch.randn((1, n, 3, 16), generator=gen) * S.sh_mask(3)
        op = 0.05 + torch.rand((1, n), generator=gen) * 0.2
        g = {"means": means, "covariances": cov, "harmonics": sh, "opacities": op}
        return (g, *_identity_camera(2.0), (64, 64))
    raise KeyError(name)


@lru_cache(maxsize=None)
def reference(name, mode, scale_invariant=True):
    """Literal-oracle render of the scene's depth (mode in MODES) or of constant colour 1 (mode
    "alpha") -> (image [V, H, W], radii [V, G], pixel flags [V, H, W], gaussian flags [V, G]); computed
    once per (scene, mode) and shared read-only."""
    g, ext, K, near, far, vps, hw = scene(name)
    rep = lambda x: x.repeat_interleave(vps, dim=0)
    means = rep(g["means"])
    if mode == "alpha":
        sh = torch.full((*means.shape[:2], 3, 1), DC_ONE)
    else:
        sh = depth_fake_color(ext, means, near, far, mode)[:, :, None, None].expand(-1, -1, 3, 1).contiguous()
    cams = prepare_cameras(ext, K, near, far, torch.zeros(ext.shape[0], 3), scale_invariant=scale_invariant)
    img, radii, _, pflag, gflag = oracle_raster.render_flagged(means, rep(g["covariances"]), sh, rep(g["opacities"]),
                                                                cams, hw, 1, 0)
    out = (img.mean(axis=1), radii, pflag, gflag)
    for a in out:
        a.setflags(write=False)
    return out


def _fused(name, device, mode="depth", color=True, alpha=False, bg=None, scale_invariant=True, **kw):
    from transplat_amd.model.decoder.hip_splatting import rasterize_with_depth

    g, ext, K, near, far, vps, hw = scene(name)
    bgv = torch.zeros(ext.shape[0], 3) if bg is None else torch.tensor(bg, dtype=torch.float32).expand(ext.shape[0], 3)
    d = lambda t: t.to(device)
    cams = prepare_cameras(d(ext), d(K), d(near), d(far), d(bgv), scale_invariant=scale_invariant)
    out = rasterize_with_depth(d(g["means"]), d(g["covariances"]), d(g["harmonics"]), d(g["opacities"]), cams, hw,
                               vps, near=d(near), far=d(far), depth_mode=mode, color=color, alpha=alpha, **kw)
    torch.cuda.synchronize()
    return out


def _check_bars(img, radii, ref, tag):
    """Prints every figure, then holds the image and the radii to the bars in the module docstring."""
    ref_img, radii_ref, pflag, gflag = ref
    img, radii = img.cpu().numpy(), radii.cpu().numpy()
    assert img.shape == ref_img.shape and radii.shape == radii_ref.shape
    scale = max(float(np.abs(ref_img).max()), 1.0)
    err = np.abs(img - ref_img)
    clear = pflag == 0
    linf = float(err[clear].max()) if clear.any() else 0.0
    n_flag, n_above = int((~clear).sum()), int((err > ATOL * scale).sum())
    bad = (radii != radii_ref) & ~gflag
    print(f"{tag}: range {float(ref_img.min()):.3g}..{float(ref_img.max()):.3g} (scale {scale:.3g}), L-inf "
          f"{linf:.3e} on {int(clear.sum())} unflagged pixels, {float(err.max()):.3e} on all; {n_flag} flagged "
          f"({n_flag / clear.size:.3%}), {n_above} above {ATOL:g} scale; radii: {int(bad.sum())} differ, "
          f"{int(gflag.sum())} of {gflag.size} ambiguous")
    assert np.isfinite(img).all()
    assert not bad.any(), f"{int(bad.sum())} radii differ (first at {np.argwhere(bad)[0]})"
    assert gflag.sum() <= MAX_AMBIGUOUS_RADII * gflag.size
    assert linf <= ATOL * scale
    assert n_flag <= MAX_FLAGGED * clear.size
    assert float(err.max()) <= FLAGGED_CAP * scale
    assert n_above <= MAX_ABOVE * err.size


# ------------------------------------------------------------------------------------ 1: parity
@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [(n, m) for n in "AB" for m in MODES] + [("C", "depth")])
def test_fused_depth_parity(device, name, mode):
    out = _fused(name, device, mode)
    _check_bars(out.depth, out.radii, reference(name, mode), f"depth {name} {mode}")
    if name == "B":
        assert (reference(name, mode)[1] == 0).any()  # near-plane culls
    if name == "B" and mode == "relative_disparity":
        assert reference(name, mode)[0].min() < 0.01  # the clamp at 0 is reached


@pytest.mark.gpu
@pytest.mark.parametrize("sort", ["count", "bitonic"])
def test_fused_depth_parity_tile_sort_ties(device, sort, monkeypatch):
    if sort == "bitonic":
        monkeypatch.setenv("TSPLAT_RASTER_SORT", "bitonic")
    out = _fused("D", device, "depth")
    _check_bars(out.depth, out.radii, reference("D", "depth"), f"depth D ({sort})")


# ------------------------------------------------------------------------------------ 2: same pass
@pytest.mark.gpu
def test_fused_color_and_depth_only_are_bit_identical(device):
    """Colour and radii of the fused call are rasterize()'s bit for bit, and the depth-only call's
    depth is the fused call's: the blend decisions and weights are the same code in every instantiation."""
    bg = (0.3, 0.6, 0.9)
    g, ext, K, near, far, vps, hw = scene("A")
    d = lambda t: t.to(device)
    cams = prepare_cameras(d(ext), d(K), d(near), d(far), d(torch.tensor(bg).expand(ext.shape[0], 3)))
    color, radii = rasterize(d(g["means"]), d(g["covariances"]), d(g["harmonics"]), d(g["opacities"]), cams, hw, vps)
    for mode in ("depth", "relative_disparity"):
        fused = _fused("A", device, mode, bg=bg, alpha=True)
        assert torch.equal(fused.color, color) and torch.equal(fused.radii, radii)
        only = _fused("A", device, mode, color=False, bg=bg)
        assert only.color is None and only.alpha is None
        assert torch.equal(only.depth, fused.depth) and torch.equal(only.radii, radii)
        assert float(fused.depth.max()) > 0.5
    assert not torch.equal(color, _fused("A", device, "depth").color)  # the background really is in the colour


# ------------------------------------------------------------------------------------ 3: alpha
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_alpha_parity(device, name):
    """alpha = 1 - T against the oracle's render of constant colour 1 over black (sum of the weights)."""
    out = _fused(name, device, "depth", alpha=True)
    _check_bars(out.alpha, out.radii, reference(name, "alpha"), f"alpha {name}")
    only = _fused(name, device, None, color=False, alpha=True)
    assert only.depth is None and only.color is None
    assert torch.equal(only.alpha, out.alpha)
    assert 0.5 < float(out.alpha.max()) <= 1.0 and float(out.alpha.min()) >= 0.0


# ------------------------------------------------------------------------------------ 4: decoder
def _decoder(device, bg=(0.2, 0.4, 0.6), **cfg):
    return DecoderSplattingHIP(DecoderSplattingHIPCfg(**cfg), SimpleNamespace(background_color=list(bg))).to(device)


def _decoder_inputs(name, device):
    g, ext, K, near, far, vps, hw = scene(name)
    b = ext.shape[0] // vps
    d = lambda t: t.to(device)
    gs = Gaussians(d(g["means"]), d(g["covariances"]), d(g["harmonics"]), d(g["opacities"]))
    cam = (d(ext).reshape(b, vps, 4, 4), d(K).reshape(b, vps, 3, 3), d(near).reshape(b, vps), d(far).reshape(b, vps))
    return gs, cam, hw


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_decoder_fused_vs_two_pass(device, mode, monkeypatch):
    """forward(depth_mode=m): depth within 1e-5 scale of the two-pass route on ALL pixels (the blend
    decisions are the same code; only d differs, z = vz / s against torch's inverse), colour
    bit-identical to forward()."""
    dec = _decoder(device)
    gs, cam, hw = _decoder_inputs("A", device)
    plain = dec(gs, *cam, hw)
    fused = dec(gs, *cam, hw, depth_mode=mode)
    only = dec.render_depth(gs, *cam, hw, mode)
    monkeypatch.setenv("TSPLAT_DEPTH_FUSED", "0")
    two = dec(gs, *cam, hw, depth_mode=mode)
    torch.cuda.synchronize()
    assert plain.depth is None and fused.depth.shape == two.depth.shape == (2, 3, *hw)
    scale = max(float(two.depth.abs().max()), 1.0)
    diff = float((fused.depth - two.depth).abs().max())
    print(f"decoder {mode}: fused vs two-pass {diff:.3e} (scale {scale:.3g}, {diff / scale:.2e} relative)")
    assert torch.equal(fused.color, plain.color) and torch.equal(two.color, plain.color)
    assert torch.equal(only, fused.depth)
    assert diff <= 1e-5 * scale


# ------------------------------------------------------------------------------------ 5: s = 1
@pytest.mark.gpu
def test_fused_depth_parity_without_scale_invariance(device):
    out = _fused("A", device, "relative_disparity", scale_invariant=False)
    _check_bars(out.depth, out.radii, reference("A", "relative_disparity", False), "depth A relative_disparity, s = 1")


# ------------------------------------------------------------------------------------ 6: graphs
@pytest.mark.gpu
def test_decoder_depth_graph_replay_with_new_inputs(device):
    """decoder(..., depth_mode="depth") captured into a hipGraph and replayed over new Gaussians and
    cameras copied into the static inputs: colour and depth are the eager ones bit for bit."""
    from transplat_amd.model.decoder.hip_splatting import check_status

    hw = (64, 64)
    dec = _decoder(device, check_overflow=False)
    sets = []
    for o in (0, 5, 9):
        t = S.make_batch(1, image_shape=hw, scene_offset=o, device=device, near=1.0 + 0.1 * o)["target"]
        g = S.make_gaussians(1, image_shape=hw, scene_offset=o)
        sets.append([g[k].to(device) for k in ("means", "covariances", "harmonics", "opacities")]
                    + [t[k].clone() for k in ("extrinsics", "intrinsics", "near", "far")])
    run = lambda s: dec(Gaussians(*s[:4]), *s[4:], hw, depth_mode="depth")
    eager = []
    for s in sets:
        out = run(s)
        eager.append((out.color.clone(), out.depth.clone()))
    static = [t.clone() for t in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static)
    for i in (0, 1, 2, 1, 0):
        for dst, src in zip(static, sets[i]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.color, eager[i][0]) and torch.equal(out.depth, eager[i][1]), i
    assert not torch.equal(eager[0][1], eager[1][1])
    check_status(device)


@pytest.mark.gpu
def test_graphed_step_returns_depth(device):
    """GraphedStep(model, example, depth_mode="depth") replays the eager test_step(depth_mode="depth")
    bit for bit, depth included (the bar of test_graph_replays_equal_eager, with its tuned library
    GEMMs), and its colour is the colour of the step without depth."""
    from transplat_amd.e2e import GraphedStep, build_model
    from transplat_amd.gemm_tuning import use_tuned_gemms

    use_tuned_gemms(device, "fp32")
    data = S.make_batch(1, image_shape=(256, 256), device=device)
    model = build_model(device, "fp32")
    plain = model.test_step(data).color.clone()
    e = model.test_step(data, depth_mode="depth")
    e_color, e_depth = e.color.clone(), e.depth.clone()
    g = GraphedStep(model, data, depth_mode="depth")
    for _ in range(2):
        r = g.run()
        torch.cuda.synchronize()
        assert r.depth.shape == (1, 3, 256, 256)
        assert torch.equal(r.color, e_color) and torch.equal(r.depth, e_depth)
    assert torch.equal(e_color, plain)
    assert torch.isfinite(e_depth).all() and float(e_depth.max()) > 0.5


# ------------------------------------------------------------------------------------ 7: EINVAL
def _capi_args(ptrs, desc=None, mode=0, **over):
    """Argument list of tsplat_raster_depth_fwd: every pointer = ptrs[name] (or ptrs['*']), then `over`."""
    names = ["means", "cov", "shs", "opacity", "viewmat", "projmat", "campos", "tanfov", "bg", "scene_scale", "near",
             "far", "mode", "out_color", "out_depth", "out_alpha", "out_radii", "workspace", "status", "stream"]
    vals = {n: ptrs.get(n, ptrs.get("*")) for n in names}
    vals["mode"], vals["stream"] = mode, None
    vals.update(over)
    desc = desc or _lib.RasterDesc(1, 1, 1, 16, 16, 1, 0, 16)
    return [ctypes.byref(desc)] + [vals[n] for n in names]


def test_einval_before_any_launch():
    """Every argument rule is checked before the first launch, so host pointers are enough here (a
    launch would fail, with another status, on a host without a device)."""
    lib = _lib.load()
    host = ctypes.create_string_buffer(4096)
    p = {"*": ctypes.addressof(host)}
    call = lambda *a, **k: lib.tsplat_raster_depth_fwd(*_capi_args(p, *a, **k))
    einval = -1
    assert call(out_color=None, out_depth=None, out_alpha=None) == einval  # no output
    for mode in (-1, 4, 1 << 20):
        assert call(mode=mode) == einval
        assert call(mode=mode, out_depth=None) == einval  # out of range even when no depth is asked for
    assert call(near=None) == einval and call(far=None) == einval  # depth needs both planes
    assert call(near=None, far=None, out_color=None, out_alpha=None) == einval
    # the rules of tsplat_raster_fwd
    for name in ("means", "cov", "shs", "opacity", "viewmat", "projmat", "campos", "tanfov", "bg", "scene_scale",
                 "out_radii", "workspace", "status"):
        assert call(**{name: None}) == einval, name
    for bad in (_lib.RasterDesc(0, 1, 1, 16, 16, 1, 0, 16), _lib.RasterDesc(1, 3, 2, 16, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 16, 1, 1, 16), _lib.RasterDesc(1, 1, 1, 16, 16, 1, 0, 0),
                _lib.RasterDesc(1, 1, 1, 16, 16, 26, 0, 16), _lib.RasterDesc(1, 33, 33, 16, 16, 1, 0, 16),
                _lib.RasterDesc(1, 1, 1, 16, 1 << 20, 1, 0, 16)):
        assert call(bad) == einval
    assert lib.tsplat_raster_depth_fwd(None, *_capi_args(p)[1:]) == einval


@pytest.mark.gpu
def test_einval_queues_nothing(device):
    """A rejected call (depth mode out of range, every buffer valid) leaves the outputs untouched; the
    same arguments with a valid mode then render."""
    lib = _lib.load()
    g, ext, K, near, far, vps, hw = scene("B")
    d = lambda t: t.to(device).float().contiguous()
    cams = prepare_cameras(d(ext), d(K), d(near), d(far), torch.zeros(3, 3, device=device))
    v, n = ext.shape[0], g["means"].shape[1]
    desc = _lib.RasterDesc(n, v, vps, *hw, g["harmonics"].shape[-1], 3, 1 << 19)  # >= G V tiles
    ws = torch.empty(int(lib.tsplat_raster_workspace_bytes(n, v, *hw, desc.capacity)), dtype=torch.uint8, device=device)
    t = {"means": d(g["means"]), "cov": d(g["covariances"]), "shs": d(g["harmonics"]), "opacity": d(g["opacities"]),
         "viewmat": cams.viewmat, "projmat": cams.projmat, "campos": cams.campos, "tanfov": cams.tanfov, "bg": cams.bg,
         "scene_scale": cams.scale, "near": d(near), "far": d(far),
         "out_color": torch.full((v, 3, *hw), -7.0, device=device), "out_depth": torch.full((v, *hw), -7.0, device=device),
         "out_alpha": torch.full((v, *hw), -7.0, device=device),
         "out_radii": torch.full((v, n), -7, dtype=torch.int32, device=device), "workspace": ws,
         "status": torch.zeros(1, dtype=torch.int32, device=device)}
    p = {k: x.data_ptr() for k, x in t.items()}
    stream = torch.cuda.current_stream(device).cuda_stream
    assert lib.tsplat_raster_depth_fwd(*_capi_args(p, desc, mode=4, stream=stream)) == -1
    torch.cuda.synchronize()
    for k in ("out_color", "out_depth", "out_alpha", "out_radii"):
        assert bool((t[k] == -7).all()), k
    assert lib.tsplat_raster_depth_fwd(*_capi_args(p, desc, mode=0, stream=stream)) == 0
    torch.cuda.synchronize()
    assert int(t["status"].item()) == 0
    for k in ("out_color", "out_depth", "out_alpha", "out_radii"):
        assert not bool((t[k] == -7).any()), k
