"""Fly-through video on the device: more than 32 views per scene through the decoder, the trajectory,
quantile and frames kernels against the float64 restatements of tests/video_ref.py, the whole tail
under hipGraph capture, and one small video end to end."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import video_ref
from transplat_amd import kernels, video
from transplat_amd import synthetic as S
from transplat_amd.misc.image_io import prep_image
from transplat_amd.model.decoder.decoder_splatting_hip import DecoderSplattingHIP, DecoderSplattingHIPCfg
from transplat_amd.model.decoder.hip_splatting import prepare_cameras, rasterize_with_depth
from transplat_amd.model.types import Gaussians
from transplat_amd.visualization.camera_trajectory.interpolation import interpolate_extrinsics

pytestmark = pytest.mark.gpu

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "video.npz")
HW = (32, 48)
BG = (0.2, 0.4, 0.6)


# ------------------------------------------------------------------------- more than 32 views
def _decoder(device, **cfg):
    return DecoderSplattingHIP(DecoderSplattingHIPCfg(**cfg), SimpleNamespace(background_color=list(BG))).to(device)


def _scene(device, scenes: int, views: int):
    """Gaussians of `scenes` scenes (G = 3,072) and `views` cameras each from the trajectory kernel:
    scene 0 runs from context view 0 to view 1, scene 1 the other way and beyond both ends."""
    g = S.make_gaussians(scenes, 2, image_shape=HW, device=device)
    ctx = S.context_extrinsics(2).to(device)
    t = torch.linspace(0, 1, views, device=device)
    ext = [interpolate_extrinsics(ctx[0], ctx[1], t), interpolate_extrinsics(ctx[1], ctx[0], t * 1.5 - 0.25)][:scenes]
    ext = torch.stack(ext)
    intr = S.intrinsics(views).to(device).expand(scenes, views, 3, 3).contiguous()
    near = torch.full((scenes, views), 1.0, device=device)
    far = torch.full((scenes, views), 100.0, device=device)
    return Gaussians(g["means"], g["covariances"], g["harmonics"], g["opacities"]), ext, intr, near, far


def _by_eights(device, gs, ext, intr, near, far):
    """The reference of the grouping: every scene on its own, 8 views per rasterize_with_depth call."""
    color, depth, radii = [], [], []
    bg = torch.tensor(BG, device=device)
    for s in range(ext.shape[0]):
        parts = []
        for v0 in range(0, ext.shape[1], 8):
            sl = slice(v0, v0 + 8)
            cams = prepare_cameras(ext[s, sl], intr[s, sl], near[s, sl], far[s, sl], bg.expand(8, 3))
            parts.append(rasterize_with_depth(gs.means[s:s + 1], gs.covariances[s:s + 1], gs.harmonics[s:s + 1],
                                              gs.opacities[s:s + 1], cams, HW, views_per_scene=8,
                                              near=near[s, sl], far=far[s, sl], depth_mode="depth"))
        color.append(torch.cat([p.color for p in parts]))
        depth.append(torch.cat([p.depth for p in parts]))
        radii.append(torch.cat([p.radii for p in parts]))
    return torch.stack(color), torch.stack(depth), torch.cat(radii)


@pytest.mark.parametrize("scenes,per_call", [(1, 16), (2, 16), (1, 7), (1, 32)])
def test_decoder_renders_more_than_32_views(device, scenes, per_call):
    """40 views per scene: colour, depth and radii of every view equal the ones of 8-view calls, so a
    view does not depend on which other views shared its call (fails on a decoder without view groups:
    the rasterizer refuses more than 32 views per scene)."""
    gs, ext, intr, near, far = _scene(device, scenes, 40)
    dec = _decoder(device, views_per_call=per_call)
    out = dec(gs, ext, intr, near, far, HW, depth_mode="depth")
    want_color, want_depth, want_radii = _by_eights(device, gs, ext, intr, near, far)
    assert out.color.shape == (scenes, 40, 3, *HW) and out.depth.shape == (scenes, 40, *HW)
    assert torch.equal(out.color, want_color)
    assert torch.equal(out.depth, want_depth)
    assert (want_depth > 0).any()  # the views see the scene
    raw = dec._render(gs, ext, intr, near, far, HW, "depth", color=True)
    assert torch.equal(raw.radii, want_radii)
    assert torch.equal(dec.render_depth(gs, ext, intr, near, far, HW), want_depth)
    assert torch.equal(dec(gs, ext, intr, near, far, HW).color, want_color)


def test_decoder_32_views_is_the_single_call(device):
    gs, ext, intr, near, far = _scene(device, 1, 32)
    out = _decoder(device)(gs, ext, intr, near, far, HW, depth_mode="depth")
    cams = prepare_cameras(ext[0], intr[0], near[0], far[0], torch.tensor(BG, device=device).expand(32, 3))
    one = rasterize_with_depth(gs.means, gs.covariances, gs.harmonics, gs.opacities, cams, HW, views_per_scene=32,
                               near=near[0], far=far[0], depth_mode="depth")
    assert torch.equal(out.color[0], one.color) and torch.equal(out.depth[0], one.depth)


# ---------------------------------------------------------------------------------- trajectory
def _check_trajectory(device, initial, final, t):
    got = kernels.trajectory_extrinsics(torch.from_numpy(initial).to(device), torch.from_numpy(final).to(device),
                                        torch.from_numpy(t).to(device)).cpu().numpy().astype(np.float64)
    want = video_ref.interpolate_extrinsics(initial, final, t)
    assert got.shape == want.shape
    # one fp32 rounding of a float64 result
    excess = np.abs(got - want) - 1.2e-7 * np.maximum(1.0, np.abs(want))
    assert excess.max() <= 0, f"trajectory kernel off by {excess.max():.3e} beyond the bound"


@pytest.mark.parametrize("name", ("smooth", "exaggerated"))
def test_trajectory_kernel_golden_cases(device, name):
    _check_trajectory(device, GOLD["traj_initial"], GOLD["traj_final"], GOLD[f"t_{name}"])
    for p in range(4):  # and each pair on its own
        _check_trajectory(device, GOLD["traj_initial"][p:p + 1], GOLD["traj_final"][p:p + 1], GOLD[f"t_{name}"])


@pytest.mark.parametrize("steps", (1, 5, 300))
def test_trajectory_kernel_three_pairs(device, steps):
    t = np.linspace(-2.0, 3.0, steps, dtype=np.float32) if steps > 1 else np.array([0.3], dtype=np.float32)
    _check_trajectory(device, GOLD["traj_initial"][:3], GOLD["traj_final"][:3], t)


def test_interpolate_extrinsics_device_path_shapes(device):
    a, b = torch.from_numpy(GOLD["traj_initial"]).to(device), torch.from_numpy(GOLD["traj_final"]).to(device)
    t = torch.from_numpy(GOLD["t_smooth"]).to(device)
    full = interpolate_extrinsics(a, b, t)
    assert full.shape == (4, 5, 4, 4) and full.is_cuda
    assert torch.equal(interpolate_extrinsics(a[1], b[1], t), full[1])


# ------------------------------------------------------------------------------------ quantile
QS = (0.0, 0.01, 0.5, 0.99, 1.0)
SIZES = (1, 2, 63, 64, 65, 257, 4099, 2 ** 20 + 3)


def _data(kind: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(n * 7 + len(kind))
    if kind == "uniform":
        return rng.random(n, dtype=np.float32)
    if kind == "equal":
        return np.full(n, 3.25, dtype=np.float32)
    if kind == "two":
        return rng.choice(np.array([1.5, -2.0], dtype=np.float32), n)
    if kind == "half_zero":
        x = rng.random(n, dtype=np.float32) + np.float32(0.5)
        x[::2] = 0
        return x
    if kind == "mixed":  # both signs, -0.0, +0.0, denormals of both signs
        x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        special = np.array([-0.0, 0.0, 1e-40, -1e-40, 1e-45, -1e-45, 3e-39], dtype=np.float32)
        idx = rng.integers(0, n, max(1, n // 3))
        x[idx] = special[rng.integers(0, special.size, idx.size)]
        return x
    if kind == "low_byte":  # the last digit pass decides
        return (np.uint32(0x40490F00) | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    raise KeyError(kind)


def _same(got: float, want: float) -> bool:
    if np.isnan(want):
        return bool(np.isnan(got))
    return abs(got - want) <= 2 * np.spacing(abs(want))


@pytest.mark.parametrize("kind", ("uniform", "equal", "two", "half_zero", "mixed", "low_byte"))
def test_quantile_kernel_matches_sort(device, kind):
    for n in SIZES:
        x = _data(kind, n)
        xd = torch.from_numpy(x).to(device)
        requests = [(q, pos) for pos in (False, True) for q in QS]
        got = torch.cat([kernels.quantile(xd, requests[i:i + 4]) for i in range(0, len(requests), 4)]).cpu().numpy()
        for (q, pos), g in zip(requests, got):
            want = video_ref.quantile(x, q, pos)
            assert _same(float(g), want), f"{kind} n={n} q={q} positive_only={pos}: {g!r} != {want!r}"


def test_quantile_kernel_requests_runs_and_alignment(device):
    x = _data("half_zero", 4099)
    xd = torch.from_numpy(x).to(device)
    requests = [(0.01, True), (0.99, False), (0.5, True), (1.0, False)]
    four = kernels.quantile(xd, requests)
    singles = torch.cat([kernels.quantile(xd, [r]) for r in requests])
    assert torch.equal(four.view(torch.int64), singles.view(torch.int64))  # bit for bit
    assert torch.equal(kernels.quantile(xd, requests).view(torch.int64), four.view(torch.int64))  # run to run
    for off in (1, 2, 3):  # a start that is not 16-byte aligned: the scalar head
        got = kernels.quantile(xd[off:], requests).cpu().numpy()
        for (q, pos), g in zip(requests, got):
            assert _same(float(g), video_ref.quantile(x[off:], q, pos))


def test_quantile_kernel_empty_positive_population(device):
    x = torch.tensor([-1.0, 0.0, -0.0, -3.5, 0.0], device=device)
    got = kernels.quantile(x, [(0.5, True), (0.5, False), (0.0, True), (1.0, False)]).cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[2])
    assert got[1] == 0.0 and got[3] == 0.0
    with pytest.raises(RuntimeError):
        kernels.quantile(x, [(1.5, False)])
    with pytest.raises(ValueError):
        kernels.quantile(x, [])


# -------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("name", ("a", "b", "const"))
def test_frames_kernel_matches_restatement(device, name):
    """Both sides are float64, so a depth pixel is excused only when r * 256 lies within 1e-6 of an
    integer; (2, 17, 23) takes the byte-store path, (3, 32, 48) the dword path."""
    color, depth = GOLD[f"frames_{name}_color"], GOLD[f"frames_{name}_depth"]
    want, r = video_ref.frames(color, depth)
    got = video.compose_frames(torch.from_numpy(color).to(device), torch.from_numpy(depth).to(device))
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    h = color.shape[2]
    assert np.array_equal(got[:, :h + 8], want[:, :h + 8])
    flag = video_ref.flagged(r, 1e-6)
    assert flag.mean() <= 0.01
    bad = (got[:, h + 8:] != want[:, h + 8:]).any(axis=-1) & ~flag
    assert not bad.any(), f"{int(bad.sum())} unflagged depth pixels differ"
    if name == "const":
        assert (got[:, h + 8:] == 0).all()
    else:
        assert (got[:, h + 8:][depth == 0] == np.array([122, 4, 2], dtype=np.uint8)).all()


@pytest.mark.parametrize("name", ("a", "b"))
def test_frames_kernel_without_depth_is_prep_image(device, name):
    color = GOLD[f"frames_{name}_color"]
    want, _ = video_ref.frames(color)
    cd = torch.from_numpy(color).to(device)
    assert np.array_equal(kernels.video_frames(cd).cpu().numpy(), want)
    assert np.array_equal(prep_image(cd[0]).cpu().numpy(), want[0])
    assert np.array_equal(prep_image(cd[0, 1]).cpu().numpy(), np.repeat(want[0][:, :, 1:2], 3, axis=2))
    side = prep_image(cd).cpu().numpy()  # a batch is laid side by side
    assert np.array_equal(side, np.concatenate(list(want), axis=1))


def test_frames_empty_positive_population_is_black(device):
    color = torch.rand((1, 3, 8, 8), device=device)
    got = video.compose_frames(color, torch.zeros((1, 8, 8), device=device)).cpu().numpy()
    assert (got[:, 16:] == 0).all() and (got[:, 8:16] == 255).all()


# ------------------------------------------------------------------------------------- capture
def test_video_tail_under_graph_capture(device):
    """Trajectory -> quantile -> frames captured in one hipGraph and replayed with new inputs: the path
    has no host sync and no pageable copy."""
    sets = []
    for i, name in enumerate(("a", "a", "a")):
        gen = torch.Generator().manual_seed(40 + i)
        color = torch.rand((3, 3, 32, 48), generator=gen) * 1.4 - 0.2
        depth = (1 + 9 * torch.rand((3, 32, 48), generator=gen)) ** (1.0 + 0.5 * i)
        depth[:, i:i + 4, 5:9] = 0
        t = torch.linspace(-0.5 * i, 1 + 0.5 * i, 5)
        sets.append([x.to(device) for x in (torch.from_numpy(GOLD["traj_initial"]).roll(i, 0),
                                            torch.from_numpy(GOLD["traj_final"]), t, color, depth)])

    def run(a, b, t, color, depth):
        return kernels.trajectory_extrinsics(a, b, t), video.compose_frames(color, depth)

    eager = [tuple(x.clone() for x in run(*s)) for s in sets]
    static = [x.clone() for x in sets[0]]
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        run(*static)
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(*static)
    for s, want in list(zip(sets, eager))[1:]:
        for dst, src in zip(static, s):
            dst.copy_(src)
        graph.replay()
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])


# ---------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(device):
    from transplat_amd.e2e import build_model

    return build_model(device)


def test_render_video_interpolation_end_to_end(device, model):
    batch = S.make_batch(1, device=device)
    seen = []
    hook = model.encoder.register_forward_hook(lambda mod, args, out: seen.append(out))
    try:
        frames = video.render_video_interpolation(model, batch, num_frames=5)
    finally:
        hook.remove()
    assert frames.dtype == torch.uint8 and not frames.is_cuda and tuple(frames.shape) == (8, 520, 256, 3)
    assert torch.equal(frames[5:], frames[[3, 2, 1]])  # loop_reverse
    assert (frames[:, 256:264] == 255).all()
    # the colour rows: prep_image of decoder.forward at the same interpolated cameras
    ctx = batch["context"]
    t = video.trajectory_times(5, True, device)
    ext = interpolate_extrinsics(ctx["extrinsics"][0, 0], ctx["extrinsics"][0, 1], t)[None]
    intr = ctx["intrinsics"][:, :1].expand(-1, 5, -1, -1)  # the synthetic views share one K
    out = model.decoder(seen[0], ext, intr, ctx["near"][:, :1].expand(-1, 5), ctx["far"][:, :1].expand(-1, 5),
                        (256, 256), depth_mode="depth")
    for i in range(5):
        assert torch.equal(frames[i, :256], prep_image(out.color[0, i]).cpu())
    assert frames[:, 264:].float().std() > 0  # a depth map, not one colour


def test_render_video_wobble_needs_two_context_views(device, model):
    batch = S.make_batch(1, num_context=3, device=device)
    assert video.render_video_wobble(model, batch) is None
    assert video.render_video_interpolation_exaggerated(model, batch) is None
