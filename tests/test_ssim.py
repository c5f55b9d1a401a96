"""SSIM of the evaluation: the HIP kernel (tsplat_ssim_fwd), compute_ssim, the per-scene plumbing of
transplat_amd.evaluate and the reference's scores files.

The oracle is `ssim_ref` below: a float64 numpy / scipy restatement of the one configuration the
reference uses (src/evaluation/metrics.py:36-52: skimage structural_similarity with win_size=11,
gaussian_weights=True, channel_axis=0, data_range=1.0), written with scipy.ndimage.gaussian_filter
itself and independent of both product paths (the torch conv2d CPU path and the kernel).

Bounds. CPU float64 path vs the restatement: 1e-12 (both float64, they differ in summation order only).
Kernel vs the restatement: 2^-23 absolute -- every intermediate of the kernel is float64 with the
restatement's weights, so the differences are summation order (~1e-13) and the one rounding of the
per-image value to fp32 (<= 2^-25 for |SSIM| <= 1); 2^-23 leaves two bits of headroom. A per-scene
value of `evaluate` is the float64 mean of the per-view fp32 values (each within 2^-25) stored once
more as fp32 in the gathered row (2^-25): within 2^-24, checked against the same 2^-23.
"""
from __future__ import annotations

import functools
import json
import math

import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

from transplat_amd import evaluate as ev
from transplat_amd.evaluation.metrics import compute_psnr, compute_ssim

BOUND = 2.0 ** -23
C1, C2 = 0.01 ** 2, 0.03 ** 2


def ssim_ref(gt: np.ndarray, pred: np.ndarray) -> np.ndarray:
    """[n, 3, H, W] pairs -> [n] float64."""
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    assert gt.shape == pred.shape and gt.ndim == 4
    h, w = gt.shape[-2:]
    if h < 11 or w < 11:
        raise ValueError("win_size exceeds image extent")
    filt = functools.partial(gaussian_filter, sigma=1.5, truncate=3.5, mode="reflect")
    cov_norm = 121.0 / 120.0
    out = np.empty(gt.shape[0], dtype=np.float64)
    for i in range(gt.shape[0]):
        maps = []
        for c in range(gt.shape[1]):
            x, y = gt[i, c], pred[i, c]
            ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
            vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
            s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
            maps.append(s[5:h - 5, 5:w - 5])
        out[i] = np.mean(np.stack(maps))
    return out


SHAPES = [(11, 11), (16, 16), (37, 53), (64, 48), (256, 256)]
KINDS = ["noisy", "scaled", "identical", "const_vs_texture"]


def _smooth(n: int, h: int, w: int, gen: torch.Generator) -> torch.Tensor:
    yy = torch.linspace(0, 1, h).reshape(1, 1, h, 1)
    xx = torch.linspace(0, 1, w).reshape(1, 1, 1, w)
    ph = torch.rand((n, 3, 1, 1), generator=gen) * 6.28
    return 0.5 + 0.35 * torch.sin(7 * xx + ph) * torch.cos(5 * yy - ph) + 0.1 * torch.rand((n, 3, h, w), generator=gen)


@functools.lru_cache(maxsize=None)
def pair(kind: str, n: int, h: int, w: int):
    """(gt, pred) fp32 CPU tensors [n, 3, h, w] and the restatement's [n] float64, computed once."""
    gen = torch.Generator().manual_seed(1000 * h + w + 17 * n + KINDS.index(kind))
    gt = _smooth(n, h, w, gen)
    if kind == "noisy":  # an unclipped render: values pushed below 0 and above 1
        gt = gt * 2 - 0.5
        pred = gt + 0.2 * torch.randn((n, 3, h, w), generator=gen)
        assert gt.min() < 0 and gt.max() > 1 and pred.min() < 0 and pred.max() > 1
    elif kind == "scaled":
        pred = gt * 0.9
    elif kind == "identical":
        pred = gt.clone()
    else:
        pred, gt = gt, torch.full_like(gt, 0.5)
    return gt, pred, ssim_ref(gt.numpy(), pred.numpy())


# ------------------------------------------------------------------------------------------- CPU


def test_restatement_anchors():
    gt, _, _ = pair("noisy", 2, 37, 53)
    assert np.array_equal(ssim_ref(gt.numpy(), gt.numpy()), np.ones(2))
    for a, b in ((0.999, 1.0), (0.25, 0.75), (0.0, 1.0)):
        x, y = np.full((1, 3, 16, 20), a), np.full((1, 3, 16, 20), b)
        assert abs(ssim_ref(x, y)[0] - (2 * a * b + C1) / (a * a + b * b + C1)) < 1e-12
    assert abs(ssim_ref(np.full((1, 3, 11, 11), 0.999), np.full((1, 3, 11, 11), 1.0))[0] - 0.99999949952) < 1e-10


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hw", SHAPES)
def test_compute_ssim_cpu_float64(hw, kind):
    gt, pred, ref = pair(kind, 2, *hw)
    got = compute_ssim(gt.double(), pred.double())
    assert got.dtype == torch.float64 and got.shape == (2,)
    err = np.abs(got.numpy() - ref).max()
    print(f"cpu ssim {hw} {kind}: max |err| {err:.3e}")
    assert err <= 1e-12


def test_compute_ssim_cpu_keeps_dtype():
    """As the reference's (torch.tensor(ssim, dtype=predicted.dtype)): fp32 in, fp32 out, one rounding."""
    gt, pred, ref = pair("noisy", 2, 37, 53)
    got = compute_ssim(gt, pred)
    assert got.dtype == torch.float32
    assert np.abs(got.double().numpy() - ref).max() <= 2.0 ** -25 + 1e-12


@pytest.mark.parametrize("hw", [(10, 16), (16, 10), (5, 5)])
def test_too_small_raises(hw):
    x = torch.rand(1, 3, *hw)
    with pytest.raises(ValueError):
        compute_ssim(x, x)
    with pytest.raises(ValueError):
        ssim_ref(x.numpy(), x.numpy())
    with pytest.raises(ValueError):
        compute_ssim(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))


def _standin(device, n_scenes=3):
    """ev.evaluate on the stand-in renderer of tests/test_distributed.py (the targets x 0.9, 16 x 16);
    returns the results and per scene the (gt, pred) CPU pairs the step saw."""
    from transplat_amd import synthetic as S

    seen = []

    def make_batch(idx, entry):
        return S.make_batch(1, image_shape=(16, 16), scene_offset=idx, device=device)

    def step(batch):
        color = batch["target"]["image"] * 0.9
        seen.append((batch["target"]["image"][0].cpu(), color[0].cpu()))
        return color

    return ev.evaluate(step, list(range(n_scenes)), make_batch, torch.device(device)), seen


def test_evaluate_fills_ssim_cpu():
    res, seen = _standin("cpu")
    assert [r.scene_idx for r in res] == [0, 1, 2]
    for r, (gt, pred) in zip(res, seen):
        ref = ssim_ref(gt.numpy(), pred.numpy()).mean()
        assert abs(r.ssim - ref) <= BOUND, (r.ssim, ref)
        assert r.psnr == pytest.approx(float(compute_psnr(gt, pred).mean()), rel=1e-6)
    s = ev.summarize(res)
    assert s["ssim"] == pytest.approx(sum(r.ssim for r in res) / 3, abs=1e-15) and 0 < s["ssim"] < 1
    assert s["psnr"] == pytest.approx(sum(r.psnr for r in res) / 3) and s["scenes"] == 3 and s["views"] == 9
    old = ev.SceneResult(4, 20.0, 3, 0.5)
    assert math.isnan(old.ssim) and old.capture is False
    assert ev.SceneResult(4, 20.0, 3, 0.5, True, 0.75).ssim == 0.75


def test_gather_results_carries_ssim():
    local = [ev.SceneResult(2, 21.5, 3, 0.25, True, 0.875), ev.SceneResult(0, 30.0, 2, 0.5, False, 0.5)]
    out = ev.gather_results(local, torch.device("cpu"), 1)
    assert [(r.scene_idx, r.psnr, r.n_views, r.seconds, r.capture, r.ssim) for r in out] == [
        (0, 30.0, 2, 0.5, False, 0.5), (2, 21.5, 3, 0.25, True, 0.875)]


def test_evaluate_stream_collects_scene_keys():
    def batches():
        for i in range(4):
            img = torch.rand((1, 2, 3, 12, 12), generator=torch.Generator().manual_seed(i))
            yield {"context": {"image": img}, "target": {"image": img}, "scene": [f"scene{i}"]}

    keys = []
    res = ev.evaluate_stream(lambda b: b["target"]["image"] * 0.9, batches(), torch.device("cpu"), keys=keys)
    assert keys == ["scene0", "scene1", "scene2", "scene3"] and len(res) == 4
    assert all(0 < r.ssim < 1 for r in res)


def test_write_scores_files(tmp_path):
    res = [ev.SceneResult(2, 20.0, 3, 0.1, False, 0.5), ev.SceneResult(0, 30.0, 3, 0.2, True, 0.75),
           ev.SceneResult(1, 25.0, 3, 0.1, False, 0.625)]
    keys = ["aaa", "bbb", "ccc", "unused"]
    out = tmp_path / "scores" / "run"
    avg = ev.write_scores(res, keys, out)
    assert sorted(p.name for p in out.iterdir()) == ["scene_all.json", "scores_all_avg.json", "scores_psnr_all.json",
                                                     "scores_ssim_all.json"]
    assert json.loads((out / "scores_psnr_all.json").read_text()) == [30.0, 25.0, 20.0]
    assert json.loads((out / "scores_ssim_all.json").read_text()) == [0.75, 0.625, 0.5]
    assert json.loads((out / "scene_all.json").read_text()) == ["aaa", "bbb", "ccc"]
    assert json.loads((out / "scores_all_avg.json").read_text()) == {"psnr": 25.0, "ssim": 0.625} == avg
    s = ev.summarize(res)
    assert s["psnr"] == 25.0 and s["ssim"] == 0.625


# ------------------------------------------------------------------------------------------- GPU


def _kernel(gt, pred, device):
    from transplat_amd import kernels as K

    return K.ssim(gt.to(device), pred.to(device))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("hw", SHAPES)
def test_kernel_matches_restatement(device, hw, n, kind):
    gt, pred, ref = pair(kind, n, *hw)
    got = _kernel(gt, pred, device)
    assert got.dtype == torch.float32 and got.shape == (n,)
    err = np.abs(got.double().cpu().numpy() - ref).max()
    print(f"ssim kernel {hw} n={n} {kind}: ref[0] {ref[0]:.9f} max |err| {err:.3e} (bound {BOUND:.3e})")
    assert err <= BOUND


@functools.lru_cache(maxsize=None)
def stress_pair(name: str):
    n, h, w = 2, 37, 53
    full = lambda v: torch.full((n, 3, h, w), v, dtype=torch.float32)
    if name == "zeros":
        gt, pred = full(0.0), full(0.0)
    elif name == "ones":
        gt, pred = full(1.0), full(1.0)
    elif name == "black_vs_white":
        gt, pred = full(0.0), full(1.0)
    elif name == "flat_0.999_vs_1":
        gt, pred = full(0.999), full(1.0)
    else:  # one 1e4 outlier pixel in the prediction of image 0
        gt, pred, _ = pair("scaled", n, h, w)
        pred = pred.clone()
        pred[0, 1, 20, 30] = 1e4
    return gt, pred, ssim_ref(gt.numpy(), pred.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["zeros", "ones", "black_vs_white", "flat_0.999_vs_1", "outlier"])
def test_kernel_value_stress(device, name):
    gt, pred, ref = stress_pair(name)
    got = _kernel(gt, pred, device).double().cpu().numpy()
    closed = {"zeros": 1.0, "ones": 1.0, "black_vs_white": C1 / (1 + C1),
              "flat_0.999_vs_1": (2 * np.float32(0.999).astype(np.float64) + C1)
              / (np.float32(0.999).astype(np.float64) ** 2 + 1 + C1)}
    if name in closed:
        assert np.abs(ref - closed[name]).max() < 1e-12
    err = np.abs(got - ref).max()
    print(f"ssim stress {name}: ref {ref} kernel {got} max |err| {err:.3e}")
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    assert err <= BOUND


@pytest.mark.gpu
def test_kernel_deterministic_and_batch_independent(device):
    gt, pred, _ = pair("noisy", 7, 37, 53)
    g, p = gt.to(device), pred.to(device)
    from transplat_amd import kernels as K

    a, b = K.ssim(g, p), K.ssim(g, p)
    assert torch.equal(a, b)
    for i in range(7):
        assert torch.equal(K.ssim(g[i:i + 1], p[i:i + 1]), a[i:i + 1]), i
    big_g, big_p, _ = pair("scaled", 7, 256, 256)
    a = K.ssim(big_g.to(device), big_p.to(device))
    assert torch.equal(K.ssim(big_g[5:6].to(device), big_p[5:6].to(device)), a[5:6])


@pytest.mark.gpu
def test_binding_rules(device):
    from transplat_amd import _lib
    from transplat_amd import kernels as K

    gt, pred, ref = pair("noisy", 7, 37, 53)
    g, p = gt.to(device), pred.to(device)
    want = K.ssim(g, p)
    # a [1, V, 3, H, W] tensor sliced along W, and an NHWC tensor seen as NCHW
    wide = torch.zeros((1, 7, 3, 37, 80), device=device)
    wide[..., 11:64] = p
    sl = wide[0, :, :, :, 11:64]
    nhwc = g.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not sl.is_contiguous() and not nhwc.is_contiguous()
    assert torch.equal(K.ssim(nhwc, sl), want)
    assert torch.equal(compute_ssim(g, p), want)  # device tensors go to the kernel
    assert np.abs(K.ssim(g.double(), p.double()).double().cpu().numpy() - ref).max() <= BOUND  # made fp32
    with pytest.raises(RuntimeError):
        K.ssim(gt, pred)  # CPU tensors
    with pytest.raises(RuntimeError):
        K.ssim(g, pred)
    with pytest.raises(ValueError):
        K.ssim(g, p[:, :, :, :52])
    with pytest.raises(ValueError):
        K.ssim(g[:, :2], p[:, :2])  # C != 3
    with pytest.raises(ValueError):
        K.ssim(g[:, :, :10], p[:, :, :10])
    # the raw C-ABI: H = 10 is TSPLAT_EINVAL before any launch, and needs no workspace
    lib = _lib.load()
    out = torch.full((1,), -7.0, device=device)
    ws = torch.zeros(64, dtype=torch.uint8, device=device)
    x = torch.rand((1, 3, 10, 16), device=device)
    stream = _lib.stream_ptr(device)
    assert lib.tsplat_ssim_fwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), 1, 10, 16, stream) == -1
    assert lib.tsplat_ssim_fwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), 1, 16, 10, stream) == -1
    assert lib.tsplat_ssim_fwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), ws.data_ptr(), 0, 16, 16, stream) == -1
    assert lib.tsplat_ssim_fwd(None, x.data_ptr(), out.data_ptr(), ws.data_ptr(), 1, 16, 16, stream) == -1
    assert lib.tsplat_ssim_fwd(x.data_ptr(), x.data_ptr(), out.data_ptr(), None, 1, 16, 16, stream) == -1
    assert lib.tsplat_ssim_workspace_bytes(1, 10, 16) == 0
    assert lib.tsplat_ssim_workspace_bytes(7, 37, 53) == 7 * 3 * 2 * 8  # 1 x 2 tiles per plane, one double each
    assert lib.tsplat_ssim_workspace_bytes(3, 256, 256) == 3 * 3 * 64 * 8
    torch.cuda.synchronize(device)
    assert float(out.item()) == -7.0  # nothing was launched


@pytest.mark.gpu
def test_evaluate_on_device(device):
    """The stand-in step through ev.evaluate on the GPU: the SSIM is queued behind the PSNR on the
    step's stream and read after the shard's one synchronisation."""
    res, seen = _standin(device)
    assert [r.scene_idx for r in res] == [0, 1, 2] and all(r.n_views == 3 for r in res)
    for r, (gt, pred) in zip(res, seen):
        ref = ssim_ref(gt.numpy(), pred.numpy()).mean()
        want_psnr = float(compute_psnr(gt.to(device), pred.to(device)).mean())
        print(f"evaluate scene {r.scene_idx}: ssim {r.ssim:.9f} ref {ref:.9f} psnr {r.psnr:.6f} want {want_psnr:.6f}")
        assert abs(r.ssim - ref) <= BOUND
        assert r.psnr == want_psnr
    assert ev.summarize(res)["ssim"] == pytest.approx(sum(r.ssim for r in res) / 3, abs=1e-15)
