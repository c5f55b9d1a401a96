"""Correlation kernels (corr.hip, uvfused.hip) on non-square and odd maps, over every depth-count
dispatch boundary and on epipolar orders that stress the run dedup, against a float64 reference
(oracle.encoder_ops with dtype=torch.float64: inputs widened before the first operation, explicit
four-corner sampling, no grid_sample) -- a mistake shared by the fp32 oracle and the kernels, which
follow the same fp32 operation order, would not show against the fp32 oracle.

Bounds: the project's own for each operation, now against float64 -- coarse and cross 1e-4 max abs
on O(1) outputs (tests/test_encoder_ops.py), msda 1e-5, depth_softmax 2e-6, the UV modules the
uv.coarse / uv.fine bounds of test_modules._GPU_TOL_DEFAULT. The CPU tests state the conditions on
the inputs that make those bounds meaningful: the fp32 oracle itself lies within 5e-5 (half the
bar) of float64 on every case, at least 0.05 of every case's outputs are non-zero, and a reference
with one of three index mistakes built in lies more than 1e-2 (100 x the bar) from the true one.

Which coarse kernel instantiation (tsplat_uv_coarse_fwd, S = ceil(D / 64)) a case reaches; every
case runs the four variants run / run6 / bitmap / direct (the launcher's table in corr.hip):
  variant   env                                        D <= 64   65..128   129..192  193..256   > 256
  run       (none)                                     run<1,8>  run<2,8>  run<3,6>  run<4,6>   plain
  run6      TSPLAT_CORR_RUN_WPE=6                      run<1,6>  run<2,6>  run<3,6>  run<4,6>   plain
  bitmap    TSPLAT_UV_COARSE_BITMAP=1                  dedup<1>  dedup<2>  dedup<3>  dedup<4>   plain
  direct    TSPLAT_UV_COARSE_DIRECT=1                  plain (uv_coarse_kernel) at every D
  S = 1: shapes 6x10 D=5, 9x11 D=33, 40x24 D=64, sweep D = 1, 15, 16, 17, 63, 64
  S = 2: shapes 12x40 D=100, 24x40 D=128, every 12x20 construction (D=100), sweep D = 65, 128
  S = 3: shapes 20x12 D=130, sweep D = 129, 192
  S = 4: shapes 12x20 D=200, 9x11 D=250, sweep D = 193, 255, 256
  plain through the default route: sweep D = 257, 260, 300 (260 and 300 also cross the 256-entry
  s_out flush of uv_coarse_kernel; the cross shape D = 260 that of uv_cross_kernel)
  partial last slice (D % 64 != 0): most of the above; p >= HW early return and partial last bitmap
  word: 9x11 (HW = 99); lane-63 -> lane-0 cell hand-off: every S >= 2 case.

Measured on MI355X (max |kernel - float64|): in each GPU test's docstring and in DESIGN.md, section 4.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_encoder_ops import GOLD, _cams, _rotated_cams, seeded  # noqa: E402

from oracle import encoder_ops as E  # noqa: E402

F64 = torch.float64
BAR = 1e-4            # the project's bound for both correlation operations (max abs, O(1) outputs)
ORACLE_BAR = 5e-5     # fp32 oracle vs float64: half the bar, so a kernel keeps room under it
MIN_SHARE = 0.05      # of the outputs non-zero (test_uv_cross_fused's figure)
MUTANT_GAP = 100 * BAR

COARSE_VARIANTS = {
    "run": {},
    "run6": {"TSPLAT_CORR_RUN_WPE": "6"},
    "bitmap": {"TSPLAT_UV_COARSE_BITMAP": "1"},
    "direct": {"TSPLAT_UV_COARSE_DIRECT": "1"},
}

# (h, w, b, D, seed of _rotated_cams' rotation or None: the synthetic batch's own poses)
SHAPES = [
    (6, 10, 1, 5, None),
    (9, 11, 1, 33, None),     # HW = 99: odd, no multiple of 4 or 32
    (12, 40, 2, 100, None),
    (20, 12, 3, 130, 4),      # odd batch
    (12, 20, 1, 200, 5),
    (9, 11, 1, 250, 6),
    (24, 40, 1, 128, 7),
    (40, 24, 2, 64, 8),
]
SWEEP = [1, 15, 16, 17, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 260, 300]
CONSTRUCTIONS = ["rot_only", "tx", "ty", "tz_minus_3", "tz_minus_median", "one_disp", "descending", "shuffled"]
CH, CW, CB, CD = 12, 20, 2, 100  # the map of the constructions

# fine cross correlation: the shapes above with (D, P) of their own (260: the direct kernel's s_out
# flush and three depth chunks of the fused one), and the constructions at (100, 4)
CROSS_SHAPES = [
    (6, 10, 1, 260, 4, None),
    (9, 11, 1, 33, 3, None),
    (12, 40, 2, 5, 4, None),
    (20, 12, 3, 130, 1, 4),
    (12, 20, 1, 70, 8, 5),
    (9, 11, 1, 100, 4, 6),
    (24, 40, 1, 5, 4, 7),
    (40, 24, 2, 33, 3, 8),
]
CROSS_ROUTES = ["table", "table_bf16", "direct", "fused"]
OFFSET_SCALE = 2.0


def _sid(c):
    return "x".join(str(v) for v in c[:2]) + "-" + "-".join(str(v) for v in c[2:])


# ------------------------------------------------------------------ inputs and references (shared)
def _shape_cams(h, w, b, d, seed):
    return _cams(b, (h, w), d) if seed is None else _rotated_cams(b, (h, w), seed, depths=d)


def _sweep_cams(d):
    """6 x 10, b = 1; above the helper's 128 disparities, those again 10 % farther each time."""
    if d <= 128:
        return _cams(1, (6, 10), d)
    intr, pose, disp = _cams(1, (6, 10))
    disp = torch.cat([disp * 0.9 ** k for k in range(-(-d // 128))], dim=1)
    return intr, pose, disp[:, :d].contiguous()


def _construction(name):
    """Cameras of one epipolar-order construction on the 12 x 20 map, b = 2, D = 100."""
    intr, pose, disp = _cams(CB, (CH, CW), CD)
    pose, disp = pose.clone(), disp.clone()
    if name == "rot_only":  # every depth of a pixel in one cell: one run
        pose = _rotated_cams(CB, (CH, CW), 11, depths=CD)[1]
        pose[:, :3, 3] = 0
    elif name in ("tx", "ty"):  # axis-aligned segments
        t = pose[:, :3, 3].clone()
        size = t.norm(dim=1) * torch.where(t[:, 0] < 0, -1.0, 1.0)
        pose[:, :3, :3] = torch.eye(3)
        pose[:, :3, 3] = 0
        pose[:, 0 if name == "tx" else 1, 3] = size
    elif name == "tz_minus_3":  # samples at the w = 1e-3 clamp
        pose[:, 2, 3] -= 3
    elif name == "tz_minus_median":  # the segment crosses the clamp part-way
        pose[:, 2, 3] -= (1 / disp).median(dim=1).values
    elif name == "one_disp":
        disp = disp[:, CD // 2:CD // 2 + 1].repeat(1, CD)
    elif name == "descending":
        disp = disp.flip(1)
    elif name == "shuffled":  # non-monotone paths
        disp = disp[:, torch.randperm(CD, generator=torch.Generator().manual_seed(7))]
    elif name == "off_image":  # no sample on the image
        pose[:, 0, 3] += 1e3
    else:
        raise KeyError(name)
    return intr, pose.contiguous(), disp.contiguous()


def _case_cams(case):
    kind = case[0]
    if kind == "shape":
        return _shape_cams(*case[1]), case[1][:3]
    if kind == "sweep":
        return _sweep_cams(case[1]), (6, 10, 1)
    return _construction(case[1]), (CH, CW, CB)


_COARSE: dict = {}


def _coarse_case(case):
    """(inputs, fp32 oracle, float64 reference) of a coarse case, computed once, never modified."""
    if case not in _COARSE:
        (intr, pose, disp), (h, w, b) = _case_cams(case)
        feat = seeded((b, 2, h * w, 128), 31)
        args = (feat, intr, pose, disp)
        _COARSE[case] = (args, (h, w), E.uv_coarse(*args, h, w), E.uv_coarse(*args, h, w, dtype=F64))
    return _COARSE[case]


_CROSS: dict = {}


def _cross_inputs(case):
    kind = case[0]
    if kind == "shape":
        h, w, b, d, p, seed = case[1]
        cams, scale = _shape_cams(h, w, b, d, seed), 1.0
    elif kind == "onehot":  # logits x 30: the point softmax near one-hot
        h, w, b, d, p = 12, 20, 1, 100, 4
        cams, scale = _rotated_cams(b, (h, w), 5, depths=d), 30.0
    else:
        h, w, b, d, p = CH, CW, CB, CD, 4
        cams, scale = _construction(case[1]), 1.0
    value = seeded((b, 2, h * w, 128), 41)
    key = seeded((b, 2, h * w, 128), 42)
    offsets = seeded((b * 2, h * w, d * p * 2), 43, OFFSET_SCALE)
    logits = seeded((b * 2, h * w, d * p), 44) * scale
    return (value, key, *cams, offsets, logits), (h, w)


def _cross_case(case, bf16_value=False):
    """(inputs, float64 reference) of a cross case; bf16_value: on the bf16-exact values."""
    k = (case, bf16_value)
    if k not in _CROSS:
        args, (h, w) = _cross_inputs(case)
        if bf16_value:
            args = (args[0].bfloat16().float(), *args[1:])
        _CROSS[k] = (args, (h, w), E.uv_cross(*args, h, w, dtype=F64))
    return _CROSS[k]


COARSE_CASES = ([pytest.param(("shape", c), id=_sid(c)) for c in SHAPES]
                + [pytest.param(("sweep", d), id=f"sweep-D{d}") for d in SWEEP]
                + [pytest.param(("construction", n), id=n) for n in CONSTRUCTIONS])
CROSS_CASES = ([pytest.param(("shape", c), id=_sid(c)) for c in CROSS_SHAPES]
               + [pytest.param(("construction", n), id=n) for n in CONSTRUCTIONS]
               + [pytest.param(("onehot",), id="onehot")])


def _maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item()


# ------------------------------------------------------------------ CPU: conditions on the inputs
def test_f64_grid_matches_reference_golden():
    g = np.load(GOLD / "calc_grid.npz")
    grid = E.calculate_grid(torch.tensor(g["intr"]), torch.tensor(g["pose"]), torch.tensor(g["disp"]), 16, 16, dtype=F64)
    assert grid.dtype == F64
    np.testing.assert_allclose(grid.numpy(), g["grid"], atol=1e-5)


def test_f64_corner_sampler_matches_grid_sample():
    """The float64 corner form equals the fp32 grid_sample form to fp32 rounding on a non-square map
    (on, at and off the border), so the two references state the same operation."""
    img = seeded((7, 5, 16), 3)
    x = seeded((400,), 4) * 4 + 2
    y = seeded((400,), 5) * 5 + 3
    x[:6] = torch.tensor([-1.0, -0.5, 0.0, 4.0, 4.5, 5.0])
    y[:6] = torch.tensor([7.0, 6.5, 6.0, 0.0, -0.5, -1.0])
    a = E.bilinear_zero(img, x, y)
    b = E.bilinear_zero_corners(img.double(), x.double(), y.double())
    assert b.dtype == F64 and _maxdiff(a, b) < 1e-5


@pytest.mark.parametrize("case", COARSE_CASES)
def test_coarse_case_conditions(case):
    _, _, ref32, ref64 = _coarse_case(case)
    dist, share = _maxdiff(ref32, ref64), (ref64 != 0).double().mean().item()
    print(f"coarse {case}: fp32 oracle vs float64 {dist:.2e}, non-zero share {share:.2f}")
    assert ref64.dtype == F64 and ref32.dtype == torch.float32
    assert dist < ORACLE_BAR
    assert share >= MIN_SHARE


def test_coarse_off_image_reference_is_zero():
    _, _, ref32, ref64 = _coarse_case(("construction", "off_image"))
    assert not ref64.any() and not ref32.any()


@pytest.mark.parametrize("case", CROSS_CASES)
def test_cross_case_conditions(case):
    args, (h, w), ref64 = _cross_case(case)
    ref32 = E.uv_cross(*args, h, w)
    dist, share = _maxdiff(ref32, ref64), (ref64 != 0).double().mean().item()
    print(f"cross {case}: fp32 oracle vs float64 {dist:.2e}, non-zero share {share:.2f}")
    assert ref64.dtype == F64 and ref32.dtype == torch.float32
    assert dist < ORACLE_BAR
    assert share >= MIN_SHARE


def _swap_bv(t, b):
    """A (v b)-ordered per-camera tensor as a kernel would see it that read index (v b) as (b v)."""
    return t.reshape(b, 2, *t.shape[1:]).transpose(0, 1).reshape(t.shape).contiguous()


def _coarse_hw_swapped(feat, intr, pose, disp, h, w):
    """uv_coarse in float64 with h and w exchanged in the sampling step (loc * size - 0.5)."""
    b, _, hw, c = feat.shape
    feat = feat.double()
    ref = E._ref3d(intr, pose, disp, h, w, b, F64)
    out = torch.empty((b * 2, hw, disp.shape[1]), dtype=F64)
    for bi in range(b):
        for vi in range(2):
            r = ref[bi * 2 + vi]
            s = E.bilinear_zero_corners(feat[bi, 1 - vi].reshape(h, w, c), r[..., 0] * h - 0.5, r[..., 1] * w - 0.5)
            out[bi * 2 + vi] = (s * feat[bi, vi][:, None, :]).sum(-1) / c ** 0.5
    return out


@pytest.mark.parametrize("shape", [pytest.param(c, id=_sid(c)) for c in SHAPES])
def test_coarse_cases_expose_index_mistakes(shape):
    """Detecting power of the inputs, on the references alone: the float64 reference with a mistake
    built in lies more than 100 x the bar from the true one."""
    (feat, intr, pose, disp), (h, w), _, ref = _coarse_case(("shape", shape))
    b = shape[2]
    mutants = {"h and w exchanged in the sampling step": _coarse_hw_swapped(feat, intr, pose, disp, h, w)}
    if disp.shape[1] > 1:
        mutants["disparities rolled by one"] = E.uv_coarse(feat, intr, pose, disp.roll(1, dims=1), h, w, dtype=F64)
    if b > 1:
        mutants["(v b) camera index read as (b v)"] = E.uv_coarse(feat, _swap_bv(intr, b), _swap_bv(pose, b),
                                                                  _swap_bv(disp, b), h, w, dtype=F64)
    for name, out in mutants.items():
        gap = _maxdiff(out, ref)
        print(f"coarse {_sid(shape)}: {name}: {gap:.2e}")
        assert gap > MUTANT_GAP, (name, gap)


def _cross_hw_swapped(value, key, intr, pose, disp, offsets, logits, h, w):
    """uv_cross in float64 with h and w exchanged in the sampling step (loc * size - 0.5)."""
    b, _, hw, c = value.shape
    d = disp.shape[1]
    p = logits.shape[-1] // d
    value, key = value.double(), key.double()
    ref = E._ref3d(intr, pose, disp, h, w, b, F64)
    off = offsets.double().reshape(b * 2, hw, d, p, 2)
    wts = torch.softmax(logits.double().reshape(b * 2, hw, d, p), -1)
    out = torch.empty((b * 2, hw, d), dtype=F64)
    chunk = max(1, 65536 // (d * p))
    for bi in range(b):
        for vi in range(2):
            n = bi * 2 + vi
            other = value[bi, 1 - vi].reshape(h, w, c)
            for q0 in range(0, hw, chunk):
                sl = slice(q0, q0 + chunk)
                loc = ref[n][sl, :, None, :] + off[n][sl] / torch.tensor([w, h], dtype=F64)
                s = E.bilinear_zero_corners(other, loc[..., 0] * h - 0.5, loc[..., 1] * w - 0.5)
                out[n, sl] = ((s * wts[n][sl][..., None]).sum(2) * key[bi, vi][sl, None, :]).mean(-1)
    return out


@pytest.mark.parametrize("shape", [pytest.param(c, id=_sid(c)) for c in CROSS_SHAPES])
def test_cross_cases_expose_index_mistakes(shape):
    """The same three mistakes for the cross operation."""
    (value, key, intr, pose, disp, offsets, logits), (h, w), ref = _cross_case(("shape", shape))
    b = shape[2]
    mutants = {"h and w exchanged in the sampling step": _cross_hw_swapped(value, key, intr, pose, disp, offsets,
                                                                          logits, h, w)}
    if disp.shape[1] > 1:
        mutants["disparities rolled by one"] = E.uv_cross(value, key, intr, pose, disp.roll(1, dims=1), offsets,
                                                          logits, h, w, dtype=F64)
    if b > 1:
        mutants["(v b) camera index read as (b v)"] = E.uv_cross(value, key, _swap_bv(intr, b), _swap_bv(pose, b),
                                                                  _swap_bv(disp, b), offsets, logits, h, w, dtype=F64)
    for name, out in mutants.items():
        gap = _maxdiff(out, ref)
        print(f"cross {_sid(shape)}: {name}: {gap:.2e}")
        assert gap > MUTANT_GAP, (name, gap)


# ------------------------------------------------------------------ GPU: coarse correlation
def _coarse_variants(K, monkeypatch, dev_args, h, w):
    """{variant: output on the CPU} of every coarse kernel variant on the same device inputs."""
    outs = {}
    for name, env in COARSE_VARIANTS.items():
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            outs[name] = K.uv_coarse(*dev_args, h, w).cpu()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("case", COARSE_CASES)
def test_uv_coarse_shapes(device, monkeypatch, case):
    """(a) - (d): every coarse kernel variant within 1e-4 of the float64 reference, and the run
    kernels equal to the bitmap kernel bit for bit wherever both are eligible (D <= 256).
    Measured on MI355X: 1.6e-6 ... 2.6e-5 over all cases and variants (the largest on 24x40 D=128;
    the dedup variants equal bit for bit, the plain kernel within 1e-6 of them), i.e. the distance
    of the fp32 oracle itself (2.0e-6 ... 3.1e-5 on the same cases): fp32 sample placement."""
    from transplat_amd import kernels as K

    args, (h, w), _, ref = _coarse_case(case)
    depths = args[3].shape[1]
    outs = _coarse_variants(K, monkeypatch, [t.to(device) for t in args], h, w)
    errs = {name: _maxdiff(out, ref) for name, out in outs.items()}
    print(f"uv_coarse {case}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert all(out.shape == ref.shape and out.dtype == torch.float32 for out in outs.values())
    assert max(errs.values()) < BAR, errs
    if depths <= 256:
        for name in ("run6", "run"):
            assert torch.equal(outs[name], outs["bitmap"]), name


@pytest.mark.gpu
def test_uv_coarse_no_sample_on_image(device, monkeypatch):
    """Cameras that put no sample on the other view's map: exact zeros from every variant."""
    from transplat_amd import kernels as K

    args, (h, w), _, ref = _coarse_case(("construction", "off_image"))
    assert not ref.any()
    outs = _coarse_variants(K, monkeypatch, [t.to(device) for t in args], h, w)
    for name, out in outs.items():
        assert out.shape == ref.shape and not out.any(), name


# ------------------------------------------------------------------ GPU: fine cross correlation
def _cross_route(K, route, dev, h, w):
    value, rest = dev[0], dev[1:]
    if route == "table":
        return K.uv_cross(value, *rest, h, w)
    if route == "table_bf16":
        return K.uv_cross(value.bfloat16(), *rest, h, w)
    if route == "direct":
        return K.uv_cross_direct(value, *rest, h, w)
    with K.dense_precision("bf16x3"):
        return K.uv_cross_fused(value, *rest, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CROSS_CASES)
def test_uv_cross_shapes(device, case):
    """(e): the fp32 table route, the bf16-value table route (on the bf16-exact values), the direct
    kernel and the fused kernel (inside the bf16x3 dense mode) within 1e-4 of the float64 reference.
    Measured on MI355X, max over the cases: table 1.6e-6, bf16 value 1.6e-6, direct 1.6e-6, fused
    1.9e-6 (fp32 oracle vs float64 on the same cases: up to 1.6e-6)."""
    from transplat_amd import kernels as K

    args, (h, w), ref = _cross_case(case)
    _, _, ref_bf16 = _cross_case(case, bf16_value=True)
    dev = [t.to(device) for t in args]
    errs = {}
    for route in CROSS_ROUTES:
        out = _cross_route(K, route, dev, h, w).cpu()
        assert out.shape == ref.shape and out.dtype == torch.float32
        errs[route] = _maxdiff(out, ref_bf16 if route == "table_bf16" else ref)
    print(f"uv_cross {case}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) < BAR, errs


# ------------------------------------------------------------------ GPU: msda
def _msda_locations(n, q, p, h, w):
    """Sampling locations in [0, 1] units: random ones (some off the map), then exact pixel centres,
    exactly 0 and 1, and values far outside."""
    loc = seeded((n, q, p, 2), 52, kind="rand") * 1.3 - 0.15
    flat = loc.reshape(n, q * p, 2)
    centres = torch.stack([(torch.arange(q * p) % w + 0.5) / w, (torch.arange(q * p) // w % h + 0.5) / h], -1)
    flat[0, ::3] = centres[::3]
    special = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.5], [0.5, 0.0], [1e4, 0.5], [0.5, -1e4],
                            [-1e4, 1e4], [1e4, 1e4]])
    k = min(len(special), q * p)
    flat[-1, :k] = special[:k]
    return flat.reshape(n, q, p, 2).contiguous()


def _msda_entry(K, entry, value, loc, wts, h, w):
    """msda through tsplat_msda_fwd, or the same call as one level and one head (head dim 128) of the
    general tsplat_ms_deform_attn_fwd."""
    if entry == "msda":
        return K.msda(value, loc, wts, h, w)
    return K.ms_deform_attn(value[:, :, None], torch.tensor([[h, w]]), torch.tensor([0]), loc[:, :, None, None],
                            wts[:, :, None, None])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["msda", "ms_deform_attn"])
@pytest.mark.parametrize("points", [1, 4, 8])
@pytest.mark.parametrize("hw", [(12, 20), (7, 5)])
def test_msda_shapes(device, hw, points, entry):
    """(f): msda on non-square maps with 1 / 4 / 8 points and 37 queries (no multiple of the 16 per
    workgroup), through its own entry point and through the general mmcv-shaped kernel (which otherwise
    sees only random locations), against the float64 reference at the existing 1e-5. The locations
    include exact pixel centres, exactly 0 and 1, and far outside. Measured on MI355X: <= 3.0e-6."""
    from transplat_amd import kernels as K

    h, w = hw
    n, q = 2, 37
    value = seeded((n, h * w, 128), 51)
    loc = _msda_locations(n, q, points, h, w)
    wts = torch.softmax(seeded((n, q, points), 53), -1)
    ref = E.msda(value, loc, wts, h, w, dtype=F64)
    assert ref.dtype == F64 and (ref != 0).double().mean().item() >= MIN_SHARE
    out = _msda_entry(K, entry, value.to(device), loc.to(device), wts.to(device), h, w).cpu()
    err = _maxdiff(out, ref)
    print(f"msda {entry} {hw} P={points}: {err:.2e}")
    assert out.shape == ref.shape and err < 1e-5, err


# ------------------------------------------------------------------ GPU: depth_softmax
def _depth_softmax_f64(logits, disp):
    pdf = torch.softmax(logits.double(), dim=1)
    n, d = logits.shape[:2]
    return (disp.double().reshape(n, d, 1, 1) * pdf).sum(1, keepdim=True), pdf.max(dim=1, keepdim=True)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0.0, 80.0])
@pytest.mark.parametrize("hw", [(1, 1), (3, 11)])
@pytest.mark.parametrize("d", [1, 7, 255, 256])
def test_depth_softmax_shapes(device, d, hw, offset):
    """(g): the depth softmax head at D = 1, 7, 255, 256 (fewer depths than slices, a ragged last
    slice, the kernel's maximum) on 1 and 33 pixels, also with the logits offset by +80, against
    float64 at test_depth_softmax_kernel's 2e-6. Measured on MI355X: <= 2.6e-7 on both outputs."""
    from transplat_amd import kernels as K

    n, (h, w) = 2, hw
    logits = seeded((n, d, h, w), 97) * 4.0 + offset
    disp = torch.linspace(0.01, 1.0, d).repeat(n, 1).reshape(n, d, 1, 1)
    rc, rm = _depth_softmax_f64(logits, disp)
    oc, om = K.depth_softmax(logits.to(device), disp.to(device))
    ec, em = _maxdiff(oc.cpu(), rc), _maxdiff(om.cpu(), rm)
    print(f"depth_softmax D={d} hw={hw} offset={offset}: coarse {ec:.2e}, pdf max {em:.2e}")
    assert ec < 2e-6 and em < 2e-6, (ec, em)


@pytest.mark.gpu
def test_depth_softmax_rejects_257_depths(device):
    from transplat_amd import kernels as K

    logits = torch.zeros((1, 257, 2, 2), device=device)
    disp = torch.linspace(0.01, 1.0, 257, device=device).reshape(1, 257, 1, 1)
    with pytest.raises(RuntimeError, match="tsplat_depth_softmax_fwd failed: invalid argument"):
        K.depth_softmax(logits, disp)


# ------------------------------------------------------------------ GPU: the UV modules, non-square
def _uv_modules(dev, cams, h, w, b):
    """UVTransformer coarse (1 layer) then fine (2 layers) as test_modules._uv builds them."""
    from canonical import canonical_init
    from transplat_amd.model.utils.uv_transformer import UVTransformer

    feats = seeded((b, 2, 128, h, w), 401).to(dev)
    coarse = canonical_init(UVTransformer(embed_dims=128, mode="coarse", num_layers=1), seed=21).eval().to(dev)
    fine = canonical_init(UVTransformer(embed_dims=128, mode="fine", num_layers=2), seed=22).eval().to(dev)
    bev_pos = seeded((b * 2, h * w, 128), 402, 0.5).to(dev)
    q0 = torch.zeros((b * 2, h * w, 128), device=dev)
    cams = tuple(t.to(dev) for t in cams)
    with torch.no_grad():
        c = coarse([feats], q0, w, h, cameras=cams)
        f = fine([feats], c, w, h, bev_pos=bev_pos, cameras=cams)
    return c.cpu(), f.cpu()


# measured on MI355X (relative to each output's scale): uv.coarse 2.09e-6 in both dense modes, uv.fine
# 1.88e-6 (fp32) / 1.12e-5 (bf16x3) -- 50x to 500x below the _GPU_TOL_DEFAULT bounds, so, as
# test_modules.GPU_TOL does, 2x the measured error rounded up to two digits, never above the default
UV_TOL = {("uv.coarse", "fp32"): 4.2e-06, ("uv.fine", "fp32"): 3.8e-06,
          ("uv.coarse", "bf16x3"): 4.2e-06, ("uv.fine", "bf16x3"): 2.3e-05}
_UV_CPU: dict = {}


def _uv_modules_cpu(monkeypatch, cams, h, w, b):
    """The same modules on the CPU with the oracle ops in place of the kernels (computed once)."""
    if not _UV_CPU:
        from transplat_amd import kernels

        with monkeypatch.context() as m:
            for name in E.KERNEL_RESTATEMENTS:
                m.setattr(kernels, name, getattr(E, name))
            _UV_CPU["out"] = _uv_modules(torch.device("cpu"), cams, h, w, b)
    return _UV_CPU["out"]


@pytest.mark.gpu
@pytest.mark.parametrize("dense", ["fp32", "bf16x3"])
def test_uv_modules_non_square(device, monkeypatch, dense):
    """(h): UVTransformer coarse then fine on a 12 x 20 map, b = 2, native non-square cameras,
    128 depths: the GPU run against the same modules on the CPU with the oracle ops swapped in,
    in both dense modes. The issue's bounds are the uv.coarse / uv.fine ones of
    test_modules._GPU_TOL_DEFAULT (1e-4 / 1e-3 relative to each output's scale); achieved on MI355X:
    uv.coarse 2.09e-6 (fp32 and bf16x3), uv.fine 1.88e-6 (fp32) and 1.12e-5 (bf16x3), so the
    asserted bounds are UV_TOL's 2x measured."""
    from test_modules import _GPU_TOL_DEFAULT, _close
    from transplat_amd import kernels as K

    h, w, b = 12, 20, 2
    cams = _cams(b, (h, w), 128)
    rc, rf = _uv_modules_cpu(monkeypatch, cams, h, w, b)
    with K.dense_precision(dense):
        c, f = _uv_modules(device, cams, h, w, b)
    for name, out, ref in (("uv.coarse", c, rc), ("uv.fine", f, rf)):
        _close(out, ref, min(UV_TOL[(name, dense)], _GPU_TOL_DEFAULT[name]), f"{name} 12x20 {dense}")
