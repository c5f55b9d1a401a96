"""LPIPS of the evaluation: the HIP kernels around the VGG16 convolutions (tsplat_lpips_scale_fwd,
tsplat_lpips_tap_fwd, tsplat_lpips_reduce_fwd), kernels.lpips, compute_lpips, the weight loader
(evaluation.lpips_vgg.LpipsVGG), the per-scene plumbing of transplat_amd.evaluate and the scores files.

The oracle is `lpips_ref` below, written from the metric's definition -- LPIPS(net="vgg"), version 0.1,
linear layers on, forward(gt, pred, normalize=True), inputs not clipped -- and independent of both
product paths: F.conv2d / F.max_pool2d in float64 for the network, numpy for the taps. The weights are
LpipsVGG.seeded(0) (random, not a metric): with them the five taps carry about 73 %, 19 %, 4.5 %, 1.5 %
and 0.7 % of the value, so every comparison is made per tap, relative to the oracle's value of that tap,
as well as on the total.

Bounds.
  CPU float64 path vs the oracle: 1e-12 relative per tap (both float64, same convolutions).
  Tap kernel alone vs float64 numpy on the same fp32 features: 2^-22 relative. The kernel's arithmetic
    is float64 on fp32 inputs, so what is left is summation order and the one rounding of the tap's value
    to fp32 (2^-24), with two bits of headroom.
  Whole metric, kernel path vs the oracle: 8 x E32 per tap, where E32 is the largest per-tap relative
    error, over all cases of WHOLE_CASES, of the oracle's own algorithm evaluated in plain torch /
    numpy fp32 on the CPU. 8: the convolutions are Winograd F(2x2, 3x3), whose transforms reassociate
    the products (tests/test_conv.py grants that kernel 2e-5 of max |y| per convolution); a torch fp32
    emulation of F(2x2, 3x3) through the network measured 2.4 x E32, so 8 leaves a factor of about 3.
  Identical pair: every tap and the total <= 1e-12 (values of distinct pairs are ~1e-3).
  A scene's value of `evaluate`: the float64 mean of the per-view values in the prediction's dtype (fp32
    for the stand-in step), stored as fp32 in the gathered row. On the CPU it is compared at 1e-12 relative
    with the oracle's per-view values taken through the same two roundings; on the GPU with the
    oracle's plain mean at the whole-metric bound.
"""
from __future__ import annotations

import functools
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from transplat_amd import evaluate as ev
from transplat_amd.evaluation.lpips_vgg import LpipsVGG
from transplat_amd.evaluation.metrics import compute_lpips, compute_psnr

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
BLOCKS = (2, 2, 3, 3, 3)  # convolutions per VGG16 block: taps after convolutions 2, 4, 7, 10, 13
TAP_BOUND = 2.0 ** -22
WINO_FACTOR = 8.0


@functools.lru_cache(maxsize=None)
def seeded_net() -> LpipsVGG:
    return LpipsVGG.seeded(0)


@functools.lru_cache(maxsize=None)
def device_net(device: str) -> LpipsVGG:
    return seeded_net().to(device)


def _features(gt: torch.Tensor, pred: torch.Tensor, net: LpipsVGG, dtype) -> list[np.ndarray]:
    """Steps 1-3: the five tapped feature maps [2n, C_k, H_k, W_k] of the gt-then-pred batch in `dtype`."""
    x = torch.cat([gt, pred]).to(dtype)
    x = 2 * x - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype).reshape(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).reshape(1, 3, 1, 1)
    taps, conv = [], 0
    for k, count in enumerate(BLOCKS):
        if k:
            x = F.max_pool2d(x, kernel_size=2, stride=2)
        for _ in range(count):
            w, b = net.convs[conv]
            x = F.relu(F.conv2d(x, w.to(dtype), b.to(dtype), stride=1, padding=1))
            conv += 1
        taps.append(x.numpy())
    return taps


def tap_ref(feat: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Step 4 on feat [2n, C, H, W] (pair i = images i and n + i) in feat's dtype -> L [n]."""
    n = feat.shape[0] // 2
    eps = feat.dtype.type(1e-10)
    f0, f1 = feat[:n], feat[n:]
    a = np.sqrt((f0 * f0).sum(axis=1, keepdims=True))
    b = np.sqrt((f1 * f1).sum(axis=1, keepdims=True))
    diff = f0 / (a + eps) - f1 / (b + eps)
    d = (w.astype(feat.dtype).reshape(1, -1, 1, 1) * diff * diff).sum(axis=1)
    return d.reshape(n, -1).mean(axis=1)


def lpips_ref(gt: torch.Tensor, pred: torch.Tensor, net: LpipsVGG, dtype=torch.float64):
    """(value [n], layers [n, 5]) as numpy arrays of `dtype` (float64: the oracle)."""
    if gt.shape != pred.shape or gt.dim() != 4 or gt.shape[1] != 3:
        raise ValueError("expected equal [n, 3, H, W] shapes")
    if gt.shape[2] < 16 or gt.shape[3] < 16:
        raise ValueError("the fourth pool leaves an empty map")
    with torch.no_grad():
        feats = _features(gt, pred, net, dtype)
    layers = np.stack([tap_ref(f, net.lins[k].numpy()) for k, f in enumerate(feats)], axis=1)
    return layers.sum(axis=1), layers


def rel_err(value, layers, ref_value, ref_layers) -> float:
    """Largest relative error over the pairs, per tap and on the total."""
    value, layers = np.asarray(value, dtype=np.float64), np.asarray(layers, dtype=np.float64)
    return float(max((np.abs(layers - ref_layers) / ref_layers).max(), (np.abs(value - ref_value) / ref_value).max()))


WHOLE_CASES = ["16x16 noisy", "17x19 noisy", "32x48 independent", "33x16 out of range", "64x96 noisy n=1"]


@functools.lru_cache(maxsize=None)
def whole_case(name: str):
    """(gt, pred) fp32 CPU tensors, the oracle's (value, layers) and the fp32 CPU run's error, once."""
    gen = torch.Generator().manual_seed(100 + WHOLE_CASES.index(name))
    h, w = (int(v) for v in name.split()[0].split("x"))
    n = 1 if name.endswith("n=1") else 2
    gt = torch.rand((n, 3, h, w), generator=gen)
    if "independent" in name:
        pred = torch.rand((n, 3, h, w), generator=gen)
    elif "out of range" in name:
        pred = 1.5 * gt - 0.25 + 0.05 * torch.randn((n, 3, h, w), generator=gen)
        assert pred.min() < 0 and pred.max() > 1
    else:
        pred = gt + 0.1 * torch.randn((n, 3, h, w), generator=gen)
    ref = lpips_ref(gt, pred, seeded_net())
    e32 = rel_err(*lpips_ref(gt, pred, seeded_net(), torch.float32), *ref)
    return gt, pred, ref, e32


@functools.lru_cache(maxsize=None)
def e32_all() -> float:
    return max(whole_case(name)[3] for name in WHOLE_CASES)


# ------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("name", WHOLE_CASES)
def test_compute_lpips_cpu_float64(name):
    gt, pred, (ref_value, ref_layers), _ = whole_case(name)
    value, layers = compute_lpips(gt.double(), pred.double(), seeded_net(), return_layers=True)
    assert value.dtype == torch.float64 and value.shape == (gt.shape[0],) and layers.shape == (gt.shape[0], 5)
    err = rel_err(value.numpy(), layers.numpy(), ref_value, ref_layers)
    share = (ref_layers / ref_value[:, None]).mean(axis=0)
    print(f"cpu lpips {name}: value {ref_value} tap shares {np.round(share, 4)} max rel err {err:.3e}")
    assert err <= 1e-12
    assert torch.equal(compute_lpips(gt.double(), pred.double(), seeded_net()), value)
    assert compute_lpips(gt, pred, seeded_net()).dtype == torch.float32  # predicted's dtype


def test_identical_pair_is_zero_cpu():
    gt = whole_case("17x19 noisy")[0]
    value, layers = compute_lpips(gt, gt.clone(), seeded_net(), return_layers=True)
    assert torch.equal(value, torch.zeros(2)) and torch.equal(layers, torch.zeros(2, 5))
    ref_value, ref_layers = lpips_ref(gt, gt.clone(), seeded_net())
    assert not ref_value.any() and not ref_layers.any()


def test_too_small_and_mismatched_raise():
    net = seeded_net()
    for hw in ((15, 16), (16, 15)):
        x = torch.rand(1, 3, *hw)
        with pytest.raises(ValueError):
            compute_lpips(x, x, net)
        with pytest.raises(ValueError):
            lpips_ref(x, x, net)
    with pytest.raises(ValueError):
        compute_lpips(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17), net)
    with pytest.raises(ValueError):
        compute_lpips(torch.rand(1, 4, 16, 16), torch.rand(1, 4, 16, 16), net)


FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
SLICES = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)


def _layout_a(net: LpipsVGG) -> dict:
    sd = {"scaling_layer.shift": torch.tensor(SHIFT).reshape(1, 3, 1, 1),
          "scaling_layer.scale": torch.tensor(SCALE).reshape(1, 3, 1, 1)}
    for i, s, (w, b) in zip(FEATURES, SLICES, net.convs):
        sd[f"net.slice{s}.{i}.weight"], sd[f"net.slice{s}.{i}.bias"] = w.clone(), b.clone()
    for k, v in enumerate(net.lins):
        sd[f"lin{k}.model.1.weight"] = v.reshape(1, -1, 1, 1).clone()
    return sd


def _layout_b(net: LpipsVGG) -> tuple[dict, dict]:
    feats = {"classifier.0.weight": torch.zeros(2, 2)}  # other keys of a VGG16 state dict are ignored
    for i, (w, b) in zip(FEATURES, net.convs):
        feats[f"features.{i}.weight"], feats[f"features.{i}.bias"] = w.clone(), b.clone()
    return feats, {f"lin{k}.model.1.weight": v.reshape(1, -1, 1, 1).clone() for k, v in enumerate(net.lins)}


def _same(a: LpipsVGG, b: LpipsVGG) -> bool:
    ta, tb = a.tensors(), b.tensors()
    return len(ta) == len(tb) == 31 and all(x.dtype == torch.float32 and torch.equal(x, y) for x, y in zip(ta, tb))


def test_weight_layouts_round_trip(tmp_path):
    net = seeded_net()
    assert _same(LpipsVGG.from_state_dict(_layout_a(net)), net)
    feats, lins = _layout_b(net)
    assert _same(LpipsVGG.from_state_dict(feats, lins), net)
    torch.save(feats, tmp_path / "vgg16.pth")
    torch.save(lins, tmp_path / "lins.pth")
    assert _same(LpipsVGG.from_files(tmp_path / "vgg16.pth", tmp_path / "lins.pth"), net)
    torch.save(_layout_a(net), tmp_path / "whole.pth")
    assert _same(LpipsVGG.from_files(tmp_path / "whole.pth"), net)
    assert _same(LpipsVGG.seeded(0), net) and not _same(LpipsVGG.seeded(1), net)
    assert all(float(v.min()) >= 0 for v in net.lins)


def test_weight_loading_errors_name_the_key():
    net = seeded_net()
    sd = _layout_a(net)
    del sd["net.slice3.14.bias"]
    with pytest.raises(KeyError, match=r"net\.slice3\.14\.bias"):
        LpipsVGG.from_state_dict(sd)
    feats, lins = _layout_b(net)
    del lins["lin4.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        LpipsVGG.from_state_dict(feats, lins)
    sd = _layout_a(net)
    sd["net.slice1.0.weight"] = torch.zeros(64, 3, 3, 2)
    with pytest.raises(ValueError, match=r"net\.slice1\.0\.weight"):
        LpipsVGG.from_state_dict(sd)
    feats, lins = _layout_b(net)
    feats["features.0.weight"] = torch.zeros(64, 3, 3, 2)
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        LpipsVGG.from_state_dict(feats, lins)
    sd = _layout_a(net)
    sd["scaling_layer.scale"] = sd["scaling_layer.scale"] + torch.tensor([0.0, 1e-3, 0.0]).reshape(1, 3, 1, 1)
    with pytest.raises(ValueError, match=r"scaling_layer\.scale"):
        LpipsVGG.from_state_dict(sd)


def _standin(device, lpips=None, n_scenes=3):
    """ev.evaluate on the stand-in renderer of tests/test_ssim.py (the targets x 0.9, 16 x 16); returns
    the results and per scene the (gt, pred) CPU pairs the step saw."""
    from transplat_amd import synthetic as S

    seen = []

    def make_batch(idx, entry):
        return S.make_batch(1, image_shape=(16, 16), scene_offset=idx, device=device)

    def step(batch):
        color = batch["target"]["image"] * 0.9
        seen.append((batch["target"]["image"][0].cpu(), color[0].cpu()))
        return color

    return ev.evaluate(step, list(range(n_scenes)), make_batch, torch.device(device), lpips=lpips), seen


def test_evaluate_fills_lpips_cpu(tmp_path):
    res, seen = _standin("cpu", lpips=seeded_net())
    assert [r.scene_idx for r in res] == [0, 1, 2]
    for r, (gt, pred) in zip(res, seen):
        assert pred.dtype == torch.float32
        views = lpips_ref(gt, pred, seeded_net())[0]
        # the scene's value as evaluate defines it: per-view values in the prediction's dtype (fp32),
        # their float64 mean, one fp32 column of the gathered row
        want = float(np.float32(views.astype(np.float32).astype(np.float64).mean()))
        print(f"scene {r.scene_idx}: lpips {r.lpips!r} want {want!r} plain float64 mean {views.mean()!r}")
        assert abs(r.lpips - want) <= 1e-12 * want
        assert abs(r.lpips - views.mean()) <= 2.0 ** -23 * views.mean()  # the two fp32 roundings, 2^-24 each
        assert r.psnr == pytest.approx(float(compute_psnr(gt, pred).mean()), rel=1e-6) and 0 < r.ssim < 1
    s = ev.summarize(res)
    assert s["lpips"] == pytest.approx(sum(r.lpips for r in res) / 3, abs=1e-15) and s["lpips"] > 0
    back = ev.gather_results(list(reversed(res)), torch.device("cpu"), 1)
    assert [(r.scene_idx, r.psnr, r.ssim, r.lpips) for r in back] == [(r.scene_idx, r.psnr, r.ssim, r.lpips) for r in res]
    avg = ev.write_scores(res, ["aaa", "bbb", "ccc"], tmp_path)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["scene_all.json", "scores_all_avg.json", "scores_lpips_all.json",
                                                          "scores_psnr_all.json", "scores_ssim_all.json"]
    assert json.loads((tmp_path / "scores_lpips_all.json").read_text()) == [r.lpips for r in res]
    assert set(avg) == {"psnr", "ssim", "lpips"} == set(json.loads((tmp_path / "scores_all_avg.json").read_text()))
    assert avg["lpips"] == sum(r.lpips for r in res) / 3


def test_scene_result_keeps_positional_meaning():
    old = ev.SceneResult(4, 20.0, 3, 0.5, True, 0.75)
    assert old.ssim == 0.75 and math.isnan(old.lpips)
    assert ev.SceneResult(4, 20.0, 3, 0.5, True, 0.75, 0.125).lpips == 0.125
    local = [ev.SceneResult(2, 21.5, 3, 0.25, True, 0.875, 0.5), ev.SceneResult(0, 30.0, 2, 0.5, False, 0.5, 0.25)]
    out = ev.gather_results(local, torch.device("cpu"), 1)
    assert [(r.scene_idx, r.psnr, r.n_views, r.seconds, r.capture, r.ssim, r.lpips) for r in out] == [
        (0, 30.0, 2, 0.5, False, 0.5, 0.25), (2, 21.5, 3, 0.25, True, 0.875, 0.5)]


def test_without_lpips_nothing_changes(tmp_path):
    res, _ = _standin("cpu")
    assert all(math.isnan(r.lpips) for r in res) and all(0 < r.ssim < 1 for r in res)
    s = ev.summarize(res)
    assert set(s) == {"scenes", "psnr", "ssim", "views", "seconds", "steady_scenes", "capture_scenes", "capture_seconds"}
    avg = ev.write_scores(res, ["aaa", "bbb", "ccc"], tmp_path)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["scene_all.json", "scores_all_avg.json", "scores_psnr_all.json",
                                                          "scores_ssim_all.json"]
    assert set(avg) == {"psnr", "ssim"} == set(json.loads((tmp_path / "scores_all_avg.json").read_text()))
    # one scene without a value (a 12 x 12 scene has an SSIM and no LPIPS) keeps the key out as well
    mixed = [ev.SceneResult(0, 30.0, 3, 0.1, False, 0.5, 0.25), ev.SceneResult(1, 30.0, 3, 0.1, False, 0.5)]
    assert "lpips" not in ev.summarize(mixed)


def test_evaluate_small_scene_reports_nan_lpips():
    def batches():
        for i in range(2):
            img = torch.rand((1, 2, 3, 12, 12), generator=torch.Generator().manual_seed(i))
            yield {"context": {"image": img}, "target": {"image": img}, "scene": [f"scene{i}"]}

    res = ev.evaluate_stream(lambda b: b["target"]["image"] * 0.9, batches(), torch.device("cpu"), lpips=seeded_net())
    assert len(res) == 2 and all(math.isnan(r.lpips) and 0 < r.ssim < 1 for r in res)


# ------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", [(16, 16), (17, 19)])
def test_scale_kernel_bit_equal(device, hw, n):
    from transplat_amd import kernels as K

    gen = torch.Generator().manual_seed(7 * hw[1] + n)
    gt = torch.randn((n, 3, *hw), generator=gen) * 2  # well outside [0, 1]
    pred = torch.rand((n, 3, *hw), generator=gen) * 3 - 1
    assert gt.min() < 0 and gt.max() > 1
    x = torch.cat([gt, pred])
    want = ((2 * x - 1) - torch.tensor(SHIFT).reshape(1, 3, 1, 1)) / torch.tensor(SCALE).reshape(1, 3, 1, 1)
    got = K.lpips_scale(gt.to(device), pred.to(device))
    assert got.dtype == torch.float32 and got.shape == (2 * n, 3, *hw)
    assert torch.equal(got.cpu(), want)


# (C, H, W, pairs, pooled): the issue's five, then a pair of 16384+ quads, where the kernel splits the
# channels 4 ways instead of 16 (even widths: 8-byte loads; odd: scalar loads and both odd edges)
TAP_SHAPES = [(64, 16, 16, 2, True), (128, 5, 7, 2, True), (256, 3, 130, 2, True), (512, 2, 2, 2, True),
              (512, 1, 1, 2, False), (64, 256, 256, 1, True), (64, 255, 259, 1, True)]


@functools.lru_cache(maxsize=None)
def tap_case(c: int, h: int, w: int, n: int):
    """Non-negative seeded features [2n, C, H, W] fp32 with all-zero pixels (in the gt image only, in the
    pred image only, in both), seeded weights [C] and the float64 value [n]."""
    gen = torch.Generator().manual_seed(c * 1000 + h * 10 + w)
    feat = torch.rand((2 * n, c, h * w), generator=gen) * torch.rand((2 * n, c, 1), generator=gen)
    px = h * w
    for i in range(n):
        if px == 1:  # one pixel per image: pair 0 has it zero in pred only, the last pair in both
            feat[n + i, :, 0] = 0
            if i == n - 1:
                feat[i, :, 0] = 0
        else:
            feat[i, :, 0] = 0
            feat[n + i, :, 1] = 0
            if px >= 6:
                feat[n + i, :, px // 2] = 0
                feat[i, :, px // 2 + 1] = 0
            feat[i, :, px - 1] = 0
            feat[n + i, :, px - 1] = 0
    feat = feat.reshape(2 * n, c, h, w)
    lin = torch.rand((c,), generator=gen) / c
    return feat, lin, tap_ref(feat.double().numpy(), lin.double().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_tap_kernel(device, shape):
    from transplat_amd import kernels as K

    c, h, w, n, pool = shape
    feat, lin, ref = tap_case(c, h, w, n)
    got, pooled = K.lpips_tap(feat.to(device), lin.to(device), pool=pool)
    torch.cuda.synchronize(device)
    got = got.double().cpu().numpy()
    assert got.shape == (n,) and np.isfinite(got).all()
    if pool:
        assert torch.equal(pooled.cpu(), F.max_pool2d(feat, 2))
    else:
        assert pooled is None
    err = np.abs(got - ref)
    print(f"tap {shape}: ref {ref} kernel {got} rel err {err / np.where(ref > 0, ref, 1)} (bound {TAP_BOUND:.3e})")
    assert (err <= TAP_BOUND * ref).all()
    if h * w == 1:
        assert ref[-1] == 0.0 and got[-1] == 0.0  # 0 / (0 + 1e-10) = 0, not NaN


@pytest.mark.gpu
def test_whole_metric_matches_oracle(device):
    """Measured on MI355X: E32 2.18e-6 (the 16 x 16 case), kernel path 7.35e-6 (same case, fifth tap),
    ratio 3.37 against the bound of 8; per case in DESIGN.md section 8b."""
    from transplat_amd import kernels as K

    net = device_net(str(device))
    worst = 0.0
    for name in WHOLE_CASES:
        gt, pred, (ref_value, ref_layers), e32 = whole_case(name)
        value, layers = K.lpips(gt.to(device), pred.to(device), net, return_layers=True)
        assert value.dtype == torch.float32 and value.shape == (gt.shape[0],) and layers.shape == (gt.shape[0], 5)
        assert torch.equal(K.lpips(gt.to(device), pred.to(device), net), value)
        err = rel_err(value.cpu().numpy(), layers.cpu().numpy(), ref_value, ref_layers)
        per_tap = (np.abs(layers.double().cpu().numpy() - ref_layers) / ref_layers).max(axis=0)
        print(f"lpips {name}: value {ref_value} E32 {e32:.3e} kernel {err:.3e} ratio {err / e32:.2f} per tap {per_tap}")
        worst = max(worst, err)
    print(f"lpips all cases: E32 {e32_all():.3e} kernel {worst:.3e} ratio {worst / e32_all():.2f} (bound {WINO_FACTOR})")
    assert worst <= WINO_FACTOR * e32_all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["17x19 noisy", "32x48 independent"])
def test_identical_pair_on_device(device, name):
    from transplat_amd import kernels as K

    g = whole_case(name)[0].to(device)
    value, layers = K.lpips(g, g.clone(), device_net(str(device)), return_layers=True)
    print(f"identical pair {name}: value {value.tolist()} layers {layers.tolist()} "
          f"exactly zero: {not bool(value.any()) and not bool(layers.any())}")
    assert float(value.abs().max()) <= 1e-12 and float(layers.abs().max()) <= 1e-12


@pytest.mark.gpu
def test_deterministic_and_batch_independent(device):
    from transplat_amd import kernels as K

    net = device_net(str(device))
    gen = torch.Generator().manual_seed(5)
    gt = torch.rand((9, 3, 16, 16), generator=gen)  # 9 pairs: a chunk of 8 and one of 1
    pred = gt + 0.1 * torch.randn((9, 3, 16, 16), generator=gen)
    g, p = gt.to(device), pred.to(device)
    assert K.LPIPS_CHUNK == 8
    a, la = K.lpips(g, p, net, return_layers=True)
    b, lb = K.lpips(g, p, net, return_layers=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    for i in range(9):
        one, lone = K.lpips(g[i:i + 1], p[i:i + 1], net, return_layers=True)
        assert torch.equal(one, a[i:i + 1]) and torch.equal(lone, la[i:i + 1]), i
    ref_value, ref_layers = lpips_ref(gt, pred, seeded_net())
    assert rel_err(a.cpu().numpy(), la.cpu().numpy(), ref_value, ref_layers) <= WINO_FACTOR * e32_all()


@pytest.mark.gpu
def test_binding_rules(device):
    from transplat_amd import _lib
    from transplat_amd import kernels as K

    net = device_net(str(device))
    gt, pred, _, _ = whole_case("17x19 noisy")
    g, p = gt.to(device), pred.to(device)
    want = K.lpips(g, p, net)
    # a [1, V, 3, H, W] tensor sliced along W, and an NHWC tensor seen as NCHW
    wide = torch.zeros((1, 2, 3, 17, 40), device=device)
    wide[..., 11:30] = p
    sl = wide[0, :, :, :, 11:30]
    nhwc = g.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not sl.is_contiguous() and not nhwc.is_contiguous()
    assert torch.equal(K.lpips(nhwc, sl, net), want)
    assert torch.equal(compute_lpips(g, p, net), want)  # device tensors go to the kernels
    got64 = compute_lpips(g.double(), p.double(), net)
    assert got64.dtype == torch.float64 and torch.equal(got64.float(), want)  # inputs made fp32
    assert K.lpips(g[:0], p[:0], net).shape == (0,)
    with pytest.raises(RuntimeError):
        K.lpips(gt, pred, net)  # CPU tensors
    with pytest.raises(RuntimeError):
        K.lpips(g, pred, net)
    with pytest.raises(RuntimeError):
        K.lpips(g, p, seeded_net())  # CPU weights
    with pytest.raises(ValueError):
        K.lpips(g, p[:, :, :, :18], net)
    with pytest.raises(ValueError):
        K.lpips(g[:, :2], p[:, :2], net)  # C != 3
    with pytest.raises(ValueError):
        K.lpips(g[:, :, :15], p[:, :, :15], net)
    # the raw C-ABI: TSPLAT_EINVAL before any launch
    lib = _lib.load()
    stream = _lib.stream_ptr(device)
    x = torch.rand((2, 3, 16, 16), device=device)
    out = torch.full((4 * 3 * 16 * 16,), -7.0, device=device)
    o, xp = out.data_ptr(), x.data_ptr()
    assert lib.tsplat_lpips_scale_fwd(None, xp, o, 2, 16, 16, stream) == -1
    assert lib.tsplat_lpips_scale_fwd(xp, None, o, 2, 16, 16, stream) == -1
    assert lib.tsplat_lpips_scale_fwd(xp, xp, None, 2, 16, 16, stream) == -1
    for n, h, w in ((0, 16, 16), (-1, 16, 16), (2, 0, 16), (2, 16, 0), (2, -3, 16)):
        assert lib.tsplat_lpips_scale_fwd(xp, xp, o, n, h, w, stream) == -1
    lin = torch.rand((3,), device=device)
    assert lib.tsplat_lpips_tap_fwd(None, lin.data_ptr(), o, o, 1, 3, 16, 16, stream) == -1
    assert lib.tsplat_lpips_tap_fwd(xp, None, o, o, 1, 3, 16, 16, stream) == -1
    assert lib.tsplat_lpips_tap_fwd(xp, lin.data_ptr(), None, o, 1, 3, 16, 16, stream) == -1
    for n, c, h, w in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, 0), (-1, 3, 16, 16)):
        assert lib.tsplat_lpips_tap_fwd(xp, lin.data_ptr(), o, o, n, c, h, w, stream) == -1
    blocks = (torch.tensor([4], dtype=torch.int32).numpy(), torch.tensor([256], dtype=torch.int64).numpy())
    bp, pp = blocks[0].ctypes.data, blocks[1].ctypes.data
    assert lib.tsplat_lpips_reduce_fwd(None, bp, pp, 1, o, None, 1, stream) == -1
    assert lib.tsplat_lpips_reduce_fwd(xp, None, pp, 1, o, None, 1, stream) == -1
    assert lib.tsplat_lpips_reduce_fwd(xp, bp, None, 1, o, None, 1, stream) == -1
    assert lib.tsplat_lpips_reduce_fwd(xp, bp, pp, 1, None, None, 1, stream) == -1
    assert lib.tsplat_lpips_reduce_fwd(xp, bp, pp, 1, o, None, 0, stream) == -1
    assert lib.tsplat_lpips_reduce_fwd(xp, bp, pp, 0, o, None, 1, stream) == -1
    assert lib.tsplat_lpips_reduce_fwd(xp, bp, pp, 9, o, None, 1, stream) == -1
    assert lib.tsplat_lpips_tap_blocks(64, 16, 16) == 4  # 64 quads, 16 per workgroup
    assert lib.tsplat_lpips_tap_blocks(512, 1, 1) == 1
    assert lib.tsplat_lpips_tap_blocks(64, 256, 256) == 256  # 16384 quads, 64 per workgroup
    assert lib.tsplat_lpips_tap_blocks(64, 0, 16) == 0
    assert lib.tsplat_lpips_workspace_bytes(2, 64, 16, 16) == 2 * 4 * 8
    assert lib.tsplat_lpips_workspace_bytes(0, 64, 16, 16) == 0
    torch.cuda.synchronize(device)
    assert bool((out == -7.0).all())  # nothing was launched


@pytest.mark.gpu
def test_evaluate_on_device(device):
    """The stand-in step through ev.evaluate on the GPU with LPIPS weights: the metric is queued behind
    the SSIM on the step's stream and read after the shard's one synchronisation; PSNR and SSIM are
    what they are without it."""
    res, seen = _standin(device, lpips=device_net(str(device)))
    plain, _ = _standin(device)
    assert [r.scene_idx for r in res] == [0, 1, 2] and all(r.n_views == 3 for r in res)
    bound = WINO_FACTOR * e32_all()
    for r, q, (gt, pred) in zip(res, plain, seen):
        ref = lpips_ref(gt, pred, seeded_net())[0].mean()
        print(f"evaluate scene {r.scene_idx}: lpips {r.lpips:.9e} ref {ref:.9e} rel err {abs(r.lpips - ref) / ref:.3e} "
              f"(bound {bound:.3e})")
        assert abs(r.lpips - ref) <= bound * ref
        assert r.psnr == q.psnr and r.ssim == q.ssim and math.isnan(q.lpips)
    assert "lpips" in ev.summarize(res) and "lpips" not in ev.summarize(plain)
