"""Value-stress tests: the softmax, normalisation and split-bf16 kernels on inputs whose VALUES are
hard, at small shapes (the other test files cover the shapes on randn data).

A. Softmax kernels under steered scores: one head-dim channel of q is a constant a = 16 and the same
   channel of k a function g(j) of the key index (multiples of 0.5, |g| <= 128: exact in bf16, so the
   steering product is exact in fp32 and in the hi / lo split) with scale * a * g spanning +-100
   natural-log units. Bound: err < B + 8 * e32, B the kernel's existing bound, e32 the error of the
   project's fp32 CPU restatement against float64 on the same input.
B. Normalisation kernels on data with mean >> sigma, a constant group and a single outlier. Bound
   (derived): B * max(1, |ref|max) + 16 * 2^-24 * max|x + pre_bias| * rstd * |gamma|max per group / row.
C. Split-bf16 products on same-sign data (a biased split adds like K there) and on rows / images
   scaled by 2^-12 .. 2^12 (judged per row / image): e3 < 2e-5 of max |y| and e3 <= etf / 8.
D. CPU checks that the inputs stress what they claim (not marked gpu).

Every reference is float64, computed here with plain torch.
"""
import functools
import math
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from canonical import seeded  # noqa: E402

from oracle import encoder_ops as E  # noqa: E402
from oracle.unet_blocks import bf16_hi, x3_ideal  # noqa: E402,F401
from test_conv import tf32_round  # noqa: E402  (the TF32 operand rounding behind every etf bar)

F = torch.nn.functional
A_STEER = 16.0
PATTERNS = ("ramp_up", "ramp_down", "spike_first", "spike_mid", "spike_last", "offset", "qzero")
U24 = 2.0 ** -24


def steer_g(pattern: str, n: int, gmax: float) -> torch.Tensor:
    """g(j) over n keys: multiples of 0.5 within +-gmax. ramp_up: the running max rises in every key
    tile; ramp_down: the first tile holds the max; spike_*: one key at +gmax (the last one lands in
    the masked partial tile); offset: +gmax on every key (softmax is invariant); qzero: g = 0."""
    j = torch.arange(n, dtype=torch.float64)
    ramp = torch.round((2 * j / max(n - 1, 1) - 1) * gmax * 2) / 2
    if pattern == "ramp_up":
        g = ramp
    elif pattern == "ramp_down":
        g = -ramp
    elif pattern.startswith("spike"):
        g = torch.zeros(n, dtype=torch.float64)
        g[{"spike_first": 0, "spike_mid": n // 2, "spike_last": n - 1}[pattern]] = gmax
    elif pattern == "offset":
        g = torch.full((n,), gmax, dtype=torch.float64)
    else:
        g = torch.zeros(n, dtype=torch.float64)
    assert (g * 2 == torch.round(g * 2)).all() and g.abs().max().item() <= 128
    return g.float()


def judge(fails, what, out, ref, bound, e32):
    """err < B + 8 e32, printed; a miss is collected so one case does not hide the next."""
    err = (out.double() - ref).abs().max().item()
    print(f"{what}: err {err:.3e}  B {bound:.3e}  e32 {e32:.3e}  (limit {bound + 8 * e32:.3e})")
    if not err < bound + 8 * e32:
        fails.append((what, err, bound, e32))


def naive_softmax_nonfinite(s: torch.Tensor) -> bool:
    """An fp32 softmax WITHOUT max subtraction on these scores gives Inf or NaN."""
    e = torch.exp(s.float())
    return not torch.isfinite(e / e.sum(-1, keepdim=True)).all().item()


# ===================================================================== A. steered softmax inputs
MHA_SHAPES = [(325, 2), (37, 2), (5, 2)]
MHA_CH, MHA_SCALE, MHA_GMAX = 7, 64 ** -0.5, 50.0  # scale * a = 2: g = +-50 is +-100 log units


@functools.lru_cache(maxsize=None)
def mha_case(n: int, heads: int, pattern: str, bias: bool):
    """(qkv as the kernel gets it, bias or None, float64 reference, e32, fp32 scores of head 0).
    With a bias the steering is applied to qkv + bias: the bias of the steered channels is 0.25, so
    (target - 0.25) + 0.25 is exact in fp32, and q = -bias gives an exact zero q."""
    full = seeded((1, n, 3 * heads * 64), 301 + n)
    f5 = full.view(1, n, 3, heads, 64)
    g = steer_g(pattern, n, MHA_GMAX)
    f5[:, :, 0, :, MHA_CH] = A_STEER
    f5[:, :, 1, :, MHA_CH] = g[None, :, None]
    if pattern == "qzero":
        f5[:, :, 0] = 0.0
    bv = None
    qkv = full
    if bias:
        bv = seeded((3 * heads * 64,), 302) * 0.5
        bv.view(3, heads, 64)[:2, :, MHA_CH] = 0.25
        qkv = full - bv
        if pattern == "qzero":
            qkv.view(1, n, 3, heads, 64)[:, :, 0] = -bv.view(3, heads, 64)[0]
    x64 = qkv.double() + bv.double() if bias else qkv.double()
    x32 = qkv + bv if bias else qkv
    src = x64
    if pattern == "offset":  # softmax is invariant: the reference is the g = 0 result
        src = x64.clone()
        src.view(1, n, 3, heads, 64)[:, :, 1, :, MHA_CH] -= MHA_GMAX
    ref = E.mha(src, heads, MHA_SCALE)
    e32 = (E.mha(x32, heads, MHA_SCALE).double() - ref).abs().max().item()
    q, k = x32.view(1, n, 3, heads, 64)[0, :, 0, 0], x32.view(1, n, 3, heads, 64)[0, :, 1, 0]
    return qkv, bv, ref, e32, (q @ k.T) * MHA_SCALE


CF_SHAPES = [(2, 1, 2, 256), (4, 1, 2, 37)]
CF_CH, CF_GMAX = 5, 35.5  # (32^-1/4)^2 * a = 2.83: g = +-35.5 is +-100.4 log units


def cf64(qkv, heads: int, views: int):
    """E.qkv_attention_cf restated in float64 (the oracle casts the scores to fp32)."""
    from einops import rearrange

    x = qkv.double()
    if views > 1:
        x = rearrange(x, "(v b) n t -> b n (v t)", v=views)
    bs, width, length = x.shape
    ch = width // (3 * heads)
    q, k, v = x.reshape(bs * heads, ch * 3, length).split(ch, dim=1)
    s = torch.einsum("bct,bcs->bts", q, k) / math.sqrt(ch)
    a = torch.einsum("bts,bcs->bct", torch.softmax(s, -1), v).reshape(bs, -1, length)
    return (rearrange(a, "b n (v t) -> (v b) n t", v=views) if views > 1 else a), s


@functools.lru_cache(maxsize=None)
def cf_case(vb: int, heads: int, views: int, t: int, pattern: str):
    """Steered before the views fold: the key index runs over view * t + i of batch b, which is row
    view * B + b of qkv."""
    qkv = seeded((vb, 3 * heads * 32, t), 311 + t)
    nb = vb // views
    g = steer_g(pattern, views * t, CF_GMAX).view(views, 1, t).expand(views, nb, t).reshape(vb, t)
    for hd in range(heads):
        qkv[:, hd * 96 + CF_CH] = A_STEER
        qkv[:, hd * 96 + 32 + CF_CH] = g
        if pattern == "qzero":
            qkv[:, hd * 96:hd * 96 + 32] = 0.0
    src = qkv
    if pattern == "offset":
        src = qkv.clone()
        for hd in range(heads):
            src[:, hd * 96 + 32 + CF_CH] = 0.0
    ref, _ = cf64(src, heads, views)
    _, s = cf64(qkv, heads, views)
    e32 = (E.qkv_attention_cf(qkv, heads, views).double() - ref).abs().max().item()
    return qkv, ref, e32, s[0].float()


DEPTH_SHAPES = [(1, 128, 8, 8), (1, 37, 9, 11), (1, 3, 4, 4)]
DEPTH_PATTERNS = PATTERNS + tuple(f"slice{s}" for s in range(8))


@functools.lru_cache(maxsize=None)
def depth_case(n: int, d: int, h: int, w: int, pattern: str):
    """The logits themselves are steered: seeded + g(depth), g within +-100. slice<s>: the spike at
    the first depth of the kernel's s-th depth slice (ceil(D / 8) depths each; D = 3 leaves slices
    empty, then the pattern is skipped). qzero: all logits equal."""
    per = -(-d // 8)
    if pattern.startswith("slice"):
        pos = int(pattern[5:]) * per
        if pos >= d:
            return None
        g = torch.zeros(d)
        g[pos] = 100.0
    else:
        g = steer_g(pattern, d, 100.0)
    base = seeded((n, d, h, w), 321 + d)
    logits = torch.full((n, d, h, w), 3.0) if pattern == "qzero" else base + g.view(1, d, 1, 1)
    disp = torch.linspace(0.01, 1.0, d).repeat(n, 1).reshape(n, d, 1, 1)
    src = base.double() if pattern == "offset" else logits.double()
    pdf = torch.softmax(src, 1)
    refs = ((disp.double() * pdf).sum(1, keepdim=True), pdf.max(1, keepdim=True)[0])
    o32 = E.depth_softmax(logits, disp)
    e32 = tuple((o.double() - r).abs().max().item() for o, r in zip(o32, refs))
    return logits, disp, refs, e32


WIN_HW, WIN_CH, WIN_GMAX = 64, 9, 71.0  # 128^-1/2 * a = 1.414: g = +-71 is +-100.4 log units


def win64(q, k, v, h: int, w: int, splits: int, shift: bool):
    """E.window_attention restated in float64 (the oracle casts q / k / v to fp32), one key view."""
    q, k, v = q.double(), k.double(), v.double()
    b, _, c = q.shape
    wh, ww = h // splits, w // splits
    pix = E._window_pixel_index(h, w, splits, wh // 2 if shift else 0, ww // 2 if shift else 0)
    out = torch.empty_like(q)
    if shift:
        reg = E._region_ids(h, w, splits)
    for bi in range(b):
        for wi in range(pix.shape[0]):
            s = q[bi, pix[wi]] @ k[bi, pix[wi]].T / math.sqrt(c)
            if shift:
                r = reg[wi]
                s = s + torch.where(r[:, None] == r[None, :], 0.0, -100.0).double()
            out[bi, pix[wi]] = torch.softmax(s, -1) @ v[bi, pix[wi]]
    return out


@functools.lru_cache(maxsize=None)
def win_inputs(pattern: str):
    """q, k, v [1, 64 * 64, 128]; g is a function of the in-window key position t of pixel (y, x),
    (y % 32) * 32 + x % 32, as in test_window_attention_bf16_growing_scores."""
    hw = WIN_HW
    q, k, v = (seeded((1, hw * hw, 128), s) for s in (331, 332, 333))
    ys, xs = torch.meshgrid(torch.arange(hw), torch.arange(hw), indexing="ij")
    t = ((ys % (hw // 2)) * (hw // 2) + xs % (hw // 2)).reshape(-1)
    q[..., WIN_CH] = A_STEER
    k[..., WIN_CH] = steer_g(pattern, hw * hw // 4, WIN_GMAX)[t]
    if pattern == "qzero":
        q = torch.zeros_like(q)
    k0 = k
    if pattern == "offset":
        k0 = k.clone()
        k0[..., WIN_CH] = 0.0
    return q, k, v, k0


@functools.lru_cache(maxsize=None)
def win_case(pattern: str, shift: bool):
    q, k, v, k0 = win_inputs(pattern)
    ref = win64(q, k0, v, WIN_HW, WIN_HW, 2, shift)
    e32 = (E.window_attention(q, k, v, WIN_HW, WIN_HW, 2, shift).double() - ref).abs().max().item()
    return q, k, v, ref, e32


@functools.lru_cache(maxsize=None)
def win_tf_err(pattern: str, shift: bool):
    """Error of TF32-rounded q / k / v in float64 (the second bar of test_window_attention_x3_kernel)."""
    q, k, v, ref, _ = win_case(pattern, shift)
    return (win64(tf32_round(q), tf32_round(k), tf32_round(v), WIN_HW, WIN_HW, 2, shift) - ref).abs().max().item()


@functools.lru_cache(maxsize=None)
def merge_case(pattern: str, shift: bool):
    """attention_merge: window attention, merge Linear, LayerNorm, + residual, in float64."""
    q, k, v, ref_attn, _ = win_case(pattern, shift)
    wm = seeded((128, 128), 334) / math.sqrt(128)
    ln = (seeded((128,), 335) * 0.1 + 1.0, seeded((128,), 336) * 0.1, 1e-5)
    r = seeded((1, WIN_HW * WIN_HW, 128), 337)
    y = F.layer_norm(ref_attn @ wm.double().T, (128,), ln[0].double(), ln[1].double(), ln[2]) + r.double()
    e32 = (E.attention_merge(q, k, v, WIN_HW, WIN_HW, 2, shift, wm, ln, residual=r).double() - y).abs().max().item()
    return wm, ln, r, y, e32


# ===================================================================== A. GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["16", "16x8", "32"])
@pytest.mark.parametrize("n,heads,bias", [(n, h, False) for n, h in MHA_SHAPES] + [(325, 2, True)])
def test_mha_steered(device, monkeypatch, form, n, heads, bias):
    """tsplat_mha_f32_fwd / tsplat_mha_bias_f32_fwd in each form (TSPLAT_MHA) under steered scores:
    B = 5e-5 absolute (measured figures: DESIGN.md, "Value stress")."""
    from transplat_amd import kernels as K

    monkeypatch.setenv("TSPLAT_MHA", form)
    fails = []
    for p in PATTERNS:
        qkv, bv, ref, e32, _ = mha_case(n, heads, p, bias)
        out = K.mha(qkv.to(device), heads, MHA_SCALE, bias=bv.to(device) if bias else None, precision="fp32").cpu()
        judge(fails, f"mha fp32 form {form} n={n} bias={bias} {p}", out, ref, 5e-5, e32)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("n,heads", MHA_SHAPES)
def test_mha_x3_steered(device, n, heads):
    """tsplat_mha_x3_fwd under steered scores: B = 1e-4 of max |ref|."""
    from transplat_amd import kernels as K

    fails = []
    for p in PATTERNS:
        qkv, _, ref, e32, _ = mha_case(n, heads, p, False)
        out = K.mha(qkv.to(device), heads, MHA_SCALE, precision="bf16x3").cpu()
        judge(fails, f"mha x3 n={n} {p}", out, ref, 1e-4 * ref.abs().max().item(), e32)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("vb,heads,views,t", CF_SHAPES)
def test_qkv_attention_cf_steered(device, vb, heads, views, t):
    """tsplat_qkv_attention_cf_fwd with the key index running over the folded views: B = 5e-5."""
    from transplat_amd import kernels as K

    fails = []
    for p in PATTERNS:
        qkv, ref, e32, _ = cf_case(vb, heads, views, t, p)
        out = K.qkv_attention_cf(qkv.to(device), heads, views).cpu()
        judge(fails, f"qkv_attention_cf {(vb, heads, views, t)} {p}", out, ref, 5e-5, e32)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,h,w", DEPTH_SHAPES)
def test_depth_softmax_steered(device, n, d, h, w):
    """tsplat_depth_softmax_fwd (8 depth slices merged with an exp(m_slice - M) rescale), the spike in
    each slice in turn, both outputs: B = 2e-6."""
    from transplat_amd import kernels as K

    fails = []
    for p in DEPTH_PATTERNS:
        case = depth_case(n, d, h, w, p)
        if case is None:
            continue
        logits, disp, refs, e32 = case
        outs = K.depth_softmax(logits.to(device), disp.to(device))
        for name, o, r, e in zip(("coarse", "pdf_max"), outs, refs, e32):
            judge(fails, f"depth_softmax {(n, d, h, w)} {p} {name}", o.cpu(), r, 2e-6, e)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "16"])
@pytest.mark.parametrize("shift", [False, True])
def test_window_attention_steered(device, monkeypatch, variant, shift):
    """tsplat_win_attn fp32 at 64 x 64, b = 1 (the key-split launch; "16": the 64-query kernel
    forced): B = 2e-4."""
    from transplat_amd import kernels as K

    if variant != "auto":
        monkeypatch.setenv("TSPLAT_WINATTN", variant)
    fails = []
    for p in PATTERNS:
        q, k, v, ref, e32 = win_case(p, shift)
        out = K.window_attention(q.to(device), k.to(device), v.to(device), WIN_HW, WIN_HW, 2, shift).cpu()
        judge(fails, f"window attention {variant} shift={shift} {p}", out, ref, 2e-4, e32)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "v1"])
@pytest.mark.parametrize("shift", [False, True])
def test_window_attention_x3_steered(device, monkeypatch, shift, variant):
    """tsplat_win_attn_x3_fwd where the launch splits the keys (the two-group kernel, and the 4-wave
    one forced by TSPLAT_WINATTN_X3=v1). B is both bars of
    test_window_attention_x3_kernel at once: 2e-4 of max(1, max |O|) (its bound for |s| up to ~10^2;
    3e-5 for the equal-scores pattern) and 1/8 of the error of TF32-rounded q / k / v."""
    from transplat_amd import kernels as K

    if variant != "auto":
        monkeypatch.setenv("TSPLAT_WINATTN_X3", variant)
    fails = []
    for p in PATTERNS:
        q, k, v, ref, e32 = win_case(p, shift)
        scale = max(1.0, ref.abs().max().item())
        bound = min((3e-5 if p == "qzero" else 2e-4) * scale, win_tf_err(p, shift) / 8)
        out = K.window_attention_x3(q.to(device), k.to(device), v.to(device), WIN_HW, WIN_HW, 2, shift).cpu()
        judge(fails, f"window attention x3 {variant} shift={shift} {p}", out, ref, bound, e32)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("dense", ["fp32", "bf16x3"])
@pytest.mark.parametrize("shift", [False, True])
def test_attention_merge_steered(device, dense, shift):
    """The key-split partials merged in the merge Linear's operand staging, with a residual: exact-fp32
    attention and merge (tsplat_win_attn_partials_fwd + tsplat_linear_f32_attn_merge_fwd), and the bf16x3
    mode's pair (tsplat_win_attn_x3_partials_fwd, bf16x3 merge products). B = 1e-3."""
    from transplat_amd import _lib
    from transplat_amd import kernels as K

    assert int(_lib.load().tsplat_win_attn_split(1, WIN_HW, WIN_HW, 1, 2)) > 1
    attn = K.auto_attention(dense)
    assert attn == dense
    fails = []
    d = lambda t: t.to(device)
    for p in PATTERNS:
        q, k, v, _, _ = win_case(p, shift)
        wm, ln, r, ref, e32 = merge_case(p, shift)
        with K.dense_precision(dense), K.attention_precision(attn):
            assert K.attention_x3_ready(1, WIN_HW, WIN_HW, 1, 2) == (dense == "bf16x3")
            out = K.attention_merge(d(q), d(k), d(v), WIN_HW, WIN_HW, 2, shift, d(wm), (d(ln[0]), d(ln[1]), ln[2]),
                                    residual=d(r)).cpu()
        judge(fails, f"attention_merge {dense} shift={shift} {p}", out, ref, 1e-3, e32)
    assert not fails, fails


# ===================================================================== B. normalisation inputs
GN_SHAPES = [((2, 32, 256, 256), 8, 0), ((2, 128, 16, 16), 8, 0), ((2, 128, 64, 64), 32, 0), ((3, 12, 5, 7), 4, 0),
             ((3, 40, 9, 7), 4, 30)]  # shape, groups, c1 of the (r1, r2) cat-residual form (0: no residual)
BF16_GN_SHAPES = [((2, 128, 16, 16), 8), ((3, 12, 5, 7), 4)]  # the bf16 in / out form
NORM_KINDS = ("shift100", "shift1000", "const", "outlier")
SIGMA = 0.3


def act64(y, act):
    return {"none": y, "silu": F.silu(y), "relu": torch.relu(y)}[act]


def norm_ref_tol(pre, gamma, eps):
    """float64 normalisation of pre [n, groups, L] (x + pre_bias) and the derived rounding term
    16 * 2^-24 * max|pre| * rstd * |gamma|max per group, as [n, groups, 1]."""
    mean = pre.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(pre.var(-1, unbiased=False, keepdim=True) + eps)
    gmax = 1.0 if gamma is None else gamma.abs().max().item()
    return (pre - mean) * rstd, 16 * U24 * pre.abs().amax(-1, keepdim=True) * rstd * gmax


def within(what, out, ref, bound, term, rmax, fails):
    """|out - ref| <= B max(1, |ref|max) + term, elementwise, with |ref|max (rmax) and the term taken per
    group / row, so an ordinary group does not hide under the largest one; prints the worst error and ratio."""
    tol = bound * rmax.clamp(min=1.0) + term
    err = (out.double() - ref).abs()
    ratio = (err / tol).max().item()
    print(f"{what}: err {err.max().item():.3e}  tol {tol.min().item():.3e}..{tol.max().item():.3e}  err/tol {ratio:.3f}")
    if not ratio <= 1.0:
        fails.append((what, err.max().item(), ratio))


@functools.lru_cache(maxsize=None)
def gn_case(shape, groups: int, kind: str, bf16: bool = False):
    """x, weight, beta, pre_bias for GroupNorm. shift<r>: x + pre_bias = mu_g + 0.3 z with mu_g / 0.3 =
    r * (1, -0.5, 2, 0.75)[g % 4], pre_bias carrying half of the mean; const: group 1 of sample 0 is
    exactly 1.5 with pre_bias (multiples of 2^-8, so the sum is exact); outlier: one 10^4 at the last
    element (the ragged chunk) of the last group of the last sample in N(0, 1) data."""
    n, c = shape[:2]
    cpg = c // groups
    z = seeded(shape, 401)
    w = seeded((c,), 402) * 0.5 + 1
    b = seeded((c,), 403) * 0.2
    bc = (1, c) + (1,) * (len(shape) - 2)
    if kind.startswith("shift"):
        fac = torch.tensor([1.0, -0.5, 2.0, 0.75])[torch.arange(groups) % 4]
        mu = (SIGMA * float(kind[5:]) * fac).repeat_interleave(cpg)
        pb = mu / 2
        x = pb.view(bc) + SIGMA * z
    elif kind == "const":
        pb = None if bf16 else torch.round(seeded((c,), 404) * 256) / 256
        x = z * 3 + 1.5
        ch = slice((1 % groups) * cpg, (1 % groups + 1) * cpg)
        x[0, ch] = 1.5 if pb is None else (1.5 - pb[ch]).view((cpg,) + (1,) * (len(shape) - 2))
    else:
        pb = None
        x = z.clone()
        x.view(n, groups, -1)[n - 1, groups - 1, -1] = 1e4
    if bf16:
        x = x.bfloat16()
    return x, w, b, pb


def gn_ref(x, groups, w, b, pb, eps, act, res):
    """(float64 reference, derived term, |ref|max), the last two per group and broadcast over its channels."""
    n, c = x.shape[:2]
    bc = (1, c) + (1,) * (x.dim() - 2)
    pre = x.double() + (pb.double().view(bc) if pb is not None else 0.0)
    yn, term = norm_ref_tol(pre.reshape(n, groups, -1), w, eps)
    y = yn.reshape(x.shape)
    if w is not None:
        y = y * w.double().view(bc) + b.double().view(bc)
    y = act64(y, act)
    if res is not None:
        y = y + res.double()
        if act == "relu":
            y = torch.relu(y)
    cpg = c // groups
    per_channel = lambda t: t.reshape(n, groups, 1).repeat_interleave(cpg, 1).reshape((n, c) + (1,) * (x.dim() - 2))
    return y, per_channel(term), per_channel(y.abs().reshape(n, groups, -1).amax(-1))


def const_is_act_beta(ref, b, groups, act):
    """The float64 result on the constant group is act(beta)."""
    c = b.numel()
    cpg = c // groups
    ch = slice((1 % groups) * cpg, (1 % groups + 1) * cpg)
    want = act64(b.double()[ch], act).view((cpg,) + (1,) * (ref.dim() - 2))
    return (ref[0, ch] - want).abs().max().item() < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["none", "silu"])
@pytest.mark.parametrize("shape,groups,c1", GN_SHAPES)
def test_group_norm_shifted(device, shape, groups, c1, act):
    """tsplat_group_norm_fwd in every form (stats + apply with many chunks, single launch, scalar path,
    cat-residual) on mean >> sigma, a constant group and one outlier: B = 2e-5 + the derived term."""
    from transplat_amd import kernels as K

    fails = []
    d = lambda t: t.to(device) if t is not None else None
    for kind in NORM_KINDS:
        x, w, b, pb = gn_case(shape, groups, kind)
        r12 = res = None
        if c1:
            r12 = (seeded((shape[0], c1) + shape[2:], 405), seeded((shape[0], shape[1] - c1) + shape[2:], 406))
            res = torch.cat(r12, 1)
        ref, term, rmax = gn_ref(x, groups, w, b, pb, 1e-5, act, res)
        if kind == "const" and not c1:
            assert const_is_act_beta(ref, b, groups, act)
        out = K.group_norm(d(x), groups, d(w), d(b), 1e-5, act, (d(r12[0]), d(r12[1])) if c1 else None, d(pb)).cpu()
        within(f"group_norm {shape} g={groups} {act} {kind}", out, ref, 2e-5, term, rmax, fails)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("shape,groups", BF16_GN_SHAPES)
def test_group_norm_bf16_shifted(device, shape, groups):
    """tsplat_group_norm_bf16_fwd (bf16 in / out, fp32 statistics) on the bf16-rounded inputs: its
    8e-3 bound (one bf16 rounding of the output) + the derived term."""
    from transplat_amd import kernels as K

    fails = []
    d = lambda t: t.to(device) if t is not None else None
    for kind in NORM_KINDS:
        x, w, b, pb = gn_case(shape, groups, kind, bf16=True)
        ref, term, rmax = gn_ref(x.float(), groups, w, b, pb, 1e-5, "silu", None)
        out = K.group_norm(d(x), groups, d(w), d(b), 1e-5, "silu", None, d(pb))
        assert out.dtype == torch.bfloat16
        within(f"group_norm bf16 {shape} g={groups} {kind}", out.float().cpu(), ref, 8e-3, term, rmax, fails)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 3, 7, 9), (2, 64, 32, 32)])
def test_instance_norm_shifted(device, shape):
    """InstanceNorm through the GroupNorm kernel with one group per channel: B = 2e-5 + the term."""
    from transplat_amd import kernels as K

    fails = []
    for kind in NORM_KINDS:
        x, _, _, pb = gn_case(shape, shape[1], kind)
        if pb is not None:  # no pre_bias entry: the input carries the whole mean
            x = x + pb.view(1, -1, 1, 1)
        ref, term, rmax = gn_ref(x, shape[1], None, None, None, 1e-5, "relu", None)
        out = K.instance_norm(x.to(device), 1e-5, "relu").cpu()
        within(f"instance_norm {shape} {kind}", out, ref, 2e-5, term, rmax, fails)
    assert not fails, fails


@functools.lru_cache(maxsize=None)
def rows_case(rows: int, dim: int, kind: str):
    """(x, y) with x + y the LayerNorm input [rows, dim]: shift<r>: mu_row + 0.3 z, y carrying half of
    the mean; const: row 1 exactly 1.5; outlier: one 10^4 at the end of the last row."""
    z = seeded((rows, dim), 411)
    if kind.startswith("shift"):
        fac = torch.tensor([1.0, -0.5, 2.0, 0.75])[torch.arange(rows) % 4]
        half = (SIGMA * float(kind[5:]) * fac / 2).view(rows, 1)
        return half + SIGMA * z, half.expand(rows, dim).contiguous()
    y = torch.zeros((rows, dim))
    if kind == "const":
        x = z * 3 + 1.5
        x[1 % rows] = 1.5
        y[:] = torch.round(seeded((rows, dim), 412) * 256) / 256
        x[1 % rows] -= y[1 % rows]
    else:
        x = z.clone()
        x[-1, -1] = 1e4
    return x, y


def ln_params(dim, eps):
    norm = torch.nn.LayerNorm(dim, eps=eps)
    with torch.no_grad():
        norm.weight.copy_(seeded((dim,), 413) * 0.1 + 1.0)
        norm.bias.copy_(seeded((dim,), 414) * 0.1)
    return norm


def ln_ref(pre, norm):
    """float64 LayerNorm of pre [rows, dim], the derived term and |ref|max per row, both [rows, 1]."""
    w, b = norm.weight.detach(), norm.bias.detach()
    yn, term = norm_ref_tol(pre[:, None, :], w, norm.eps)
    y = yn[:, 0] * w.double() + b.double()
    return y, term[:, 0], y.abs().amax(-1, keepdim=True)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,dim", [(33, 1024), (7, 256)])
def test_residual_ln_shifted(device, rows, dim):
    """tsplat_residual_ln_fwd (x + y, LayerNorm): the sum within 1e-5 of max(1, |x + y|max) and the norm
    within B = 2e-5 + the derived term (eps 1e-6: rstd = 1000 on the constant row)."""
    from transplat_amd import kernels as K

    norm = ln_params(dim, 1e-6)
    fails = []
    for kind in NORM_KINDS:
        x, y = rows_case(rows, dim, kind)
        pre = x.double() + y.double()
        ref, term, rmax = ln_ref(pre, norm)
        if kind == "const":
            assert (ref[1 % rows] - norm.bias.detach().double()).abs().max().item() < 1e-12
        ox, on = K.residual_ln(x.to(device), y.to(device), None, norm.to(device))
        norm.cpu()
        ex = (ox.cpu().double() - pre).abs().max().item()
        print(f"residual_ln {(rows, dim)} {kind}: sum err {ex:.3e}")
        if not ex < 1e-5 * max(1.0, pre.abs().max().item()):
            fails.append((kind, "sum", ex))
        within(f"residual_ln {(rows, dim)} {kind}", on.cpu(), ref, 2e-5, term, rmax, fails)
    assert not fails, fails


@pytest.mark.gpu
def test_layer_norm128_shifted(device):
    """tsplat_layer_norm128_fwd at (3, 1001, 128), fp32: B = 2e-5 + the derived term."""
    from transplat_amd import kernels as K

    norm = ln_params(128, 1e-5)
    fails = []
    for kind in NORM_KINDS:
        x, y = rows_case(3 * 1001, 128, kind)
        pre32 = x + y
        ref, term, rmax = ln_ref(pre32.double(), norm)
        out = K.layer_norm128(pre32.view(3, 1001, 128).to(device), norm.to(device)).cpu().view(-1, 128)
        norm.cpu()
        within(f"layer_norm128 {kind}", out, ref, 2e-5, term, rmax, fails)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("dense", ["fp32", "bf16x3"])
@pytest.mark.parametrize("res_pre_ln", [False, True])
def test_fused_linear_ln_shifted(device, dense, res_pre_ln):
    """fused_linear's LayerNorm epilogue (N = 128, K = 128, M = 257) on rows whose mean comes from a
    constant bias of 300 (sigma ~ 1); row 0 of x is zero, so its pre-norm row is constant and (plain
    form) the result there is beta. B = 2e-4 + the derived term."""
    from transplat_amd import kernels as K

    m = 257
    x = seeded((m, 128), 421)
    x[0] = 0.0
    w = seeded((128, 128), 422) / math.sqrt(128)
    bias = torch.full((128,), 300.0)
    norm = ln_params(128, 1e-5)
    g, bt = norm.weight.detach(), norm.bias.detach()
    r = seeded((m, 128), 423) if res_pre_ln else None
    pre = x.double() @ w.double().T + 300.0 + (r.double() if res_pre_ln else 0.0)
    ref, term, rmax = ln_ref(pre, norm)
    if not res_pre_ln:
        assert (ref[0] - bt.double()).abs().max().item() < 1e-12
    d = lambda t: t.to(device) if t is not None else None
    with K.dense_precision(dense):
        out = K.fused_linear(d(x), d(w), bias=d(bias), ln=(d(g), d(bt), 1e-5), residual=d(r),
                             res_pre_ln=res_pre_ln).cpu()
    fails = []
    within(f"fused_linear ln {dense} res_pre_ln={res_pre_ln}", out, ref, 2e-4, term, rmax, fails)
    assert not fails, fails


# ===================================================================== C. split-bf16 products
# (bf16_hi and x3_ideal, the ideal split in float64, are shared with the U-Net block tests:
# oracle/unet_blocks.py)
# name -> (kind, geometry): gemm (m, k, n, ksplit); conv (n, c1, c2, h, w, co, k, stride)
C_CASES = {
    "gemm_130_200_260": ("gemm", (130, 200, 260, 2)),
    "gemm_33_72_100": ("gemm", (33, 72, 100, 1)),
    "gemm_650_3072_768": ("gemm", (650, 3072, 768, 4)),            # test_gemm_x3_kernel's long reduction
    "linear_257_128_128": ("linear", (257, 128, 128, 1)),
    "linear_257_1024_128": ("linear", (257, 1024, 128, 1)),
    "direct_1x1": ("direct", (2, 128, 128, 32, 32, 128, 1, 1)),   # X3_CASES' 1x1 skip convolution
    "direct_3x3": ("direct", (2, 768, 0, 18, 18, 768, 3, 2)),      # X3_CASES' 3x3 that conv_x3_wins admits
    "wino_38_32": ("wino", (1, 38, 0, 17, 21, 32, 3, 1)),
    "wino_16_16": ("wino", (3, 16, 0, 9, 70, 16, 3, 1)),
    "wino_128_128": ("wino", (1, 128, 0, 18, 18, 128, 3, 1)),
    "few_128_16": ("few", (3, 96, 32, 20, 68, 16, 3, 1)),
}


# the cases whose reduction is long enough that a truncated split fails etf / 8 on same-sign data
# (one per kernel family; see test_ideal_split_meets_the_bars_and_truncation_does_not)
TRUNCATION_SHOWS = ("gemm_650_3072_768", "linear_257_1024_128", "direct_3x3", "wino_128_128", "few_128_16")
assert {C_CASES[c][0] for c in TRUNCATION_SHOWS} == {k for k, _ in C_CASES.values()}


def c_op(name):
    kind, geo = C_CASES[name]
    if kind in ("gemm", "linear"):
        return lambda x, w: x.double() @ w.double().T
    k, stride = geo[6], geo[7]
    return lambda x, w: F.conv2d(x.double(), w.double(), None, stride, k // 2)


@functools.lru_cache(maxsize=None)
def c_case(name: str, data: str):
    """(x, w, float64 reference, float64 result on TF32-rounded operands). same: x = |randn|,
    w = |randn| / K; scaled: zero-mean data, row i (GEMM) or image i (convolution; single-image cases
    get three images) times 2^e_i with e covering -12 .. 12. No bias."""
    kind, geo = C_CASES[name]
    if kind in ("gemm", "linear"):
        m, kk, n, _ = geo
        xs, ws, red = (m, kk), (n, kk), kk
    else:
        nb, c1, c2, h, w_, co, k, _ = geo
        nb = max(nb, 3) if data == "scaled" else nb
        xs, ws, red = (nb, c1 + c2, h, w_), (co, c1 + c2, k, k), (c1 + c2) * k * k
    x, w = seeded(xs, 501), seeded(ws, 502)
    if data == "same":
        x, w = x.abs(), w.abs() / red
    else:
        rows = xs[0]
        e = (torch.arange(rows) % 25 - 12) if rows >= 25 else torch.linspace(-12, 12, rows).round()
        x = x * torch.pow(2.0, e.float()).view((rows,) + (1,) * (len(xs) - 1))
        w = w / math.sqrt(red)
    op = c_op(name)
    return x, w, op(x, w), op(tf32_round(x), tf32_round(w))


def c_bars(out, ref, ref_tf, per_row: bool):
    """(e3, etf) relative to max |ref|: over the whole output, or per row / image against its own."""
    dims = tuple(range(1, ref.dim())) if per_row else tuple(range(ref.dim()))
    scale = ref.abs().amax(dims)
    return (out.double() - ref).abs().amax(dims) / scale, (ref_tf - ref).abs().amax(dims) / scale


def c_run(name, x, w, device, monkeypatch):
    """The case's kernel on x, w (no bias)."""
    import ctypes

    from transplat_amd import _lib
    from transplat_amd import kernels as K

    kind, geo = C_CASES[name]
    xd, wd = x.to(device), w.to(device)
    if kind == "gemm":
        with K.dense_precision("bf16x3"):
            assert K.gemm_x3_ok(xd, wd)
            y = K.gemm_x3(xd, wd, None, ksplit=geo[3])
        return (y.double().sum(0) if geo[3] > 1 else y.double()).cpu()
    if kind == "linear":
        with K.dense_precision("bf16x3"):
            return K.fused_linear(xd, wd).cpu()
    nb, (c1, c2, h, w_, co, k, stride) = x.shape[0], geo[1:]
    if kind == "direct":
        hout = (h + 2 * (k // 2) - k) // stride + 1
        wout = (w_ + 2 * (k // 2) - k) // stride + 1
        assert K.conv_x3_wins(nb * hout * wout, c1 + c2, co, k)
        with K.dense_precision("bf16x3"):
            return K.conv2d_direct(xd[:, :c1].contiguous(), wd, None, stride,
                                   x2=xd[:, c1:].contiguous() if c2 else None).cpu()
    if kind == "wino":
        monkeypatch.setattr(K, "_FEW", False)
        return K.conv3x3_wino(xd, wd, None, "none", precision="bf16x3").cpu()
    lib = _lib.load()  # the few-channel direct kernel, as test_conv3x3_few_kernel calls it
    assert int(lib.tsplat_conv3x3_few_form(nb, c1 + c2, h, w_, co)) != 0
    srcs = [xd[:, :c1].contiguous(), xd[:, c1:].contiguous()]
    y = torch.empty((nb, co, h, w_), device=device)
    ptrs = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in srcs])
    cs = (ctypes.c_int32 * 2)(c1, c2)
    rc = lib.tsplat_conv3x3_few_bf16x3_fwd(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(cs, ctypes.c_void_p), 2,
                                           K.conv_pack_weight_x3(wd).data_ptr(), None, None, None, y.data_ptr(),
                                           nb, h, w_, co, 0, 0, _lib.stream_ptr(device))
    assert rc == 0
    return y.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("data", ["same", "scaled"])
@pytest.mark.parametrize("name", list(C_CASES))
def test_split_products_value_stress(device, monkeypatch, name, data):
    """gemm_x3, fused_linear (bf16x3), the direct and Winograd bf16x3 convolutions and the few-channel
    kernel: e3 < 2e-5 of max |y| and e3 <= etf / 8, over the whole output on same-sign data and per
    row / image, each against its own max |ref|, on scaled data."""
    x, w, ref, ref_tf = c_case(name, data)
    out = c_run(name, x, w, device, monkeypatch)
    e3, etf = c_bars(out, ref, ref_tf, data == "scaled")
    worst = (e3 / etf).argmax() if e3.dim() else None
    print(f"split products {name} {data}: e3 {e3.max().item():.3e}  etf {etf.min().item():.3e}..{etf.max().item():.3e}"
          f"  worst e3/etf {(e3 / etf).max().item():.4f}" + (f" (row {int(worst)})" if worst is not None else ""))
    assert (e3 < 2e-5).all(), e3.max().item()
    assert (e3 <= etf / 8).all(), ((e3 / etf).max().item(),)


# ===================================================================== D. the inputs stress what they claim
def _softmax_inputs():
    for n, heads in MHA_SHAPES:
        for p in PATTERNS:
            c = mha_case(n, heads, p, False)
            yield f"mha n={n} {p}", p, c[4], c[2]
    for p in PATTERNS:
        c = mha_case(325, 2, p, True)
        yield f"mha bias {p}", p, c[4], c[2]
    for shp in CF_SHAPES:
        for p in PATTERNS:
            c = cf_case(*shp, p)
            yield f"cf {shp} {p}", p, c[3], c[1]
    for shp in DEPTH_SHAPES:
        for p in DEPTH_PATTERNS:
            c = depth_case(*shp, p)
            if c is not None:
                yield f"depth {shp} {p}", p, c[0].permute(0, 2, 3, 1), torch.cat(c[2])
    for p in PATTERNS:
        q, k, v, ref, _ = win_case(p, False)
        pix = E._window_pixel_index(WIN_HW, WIN_HW, 2, 0, 0)[0]
        yield f"window {p}", p, q[0, pix] @ k[0, pix].T / math.sqrt(128), ref


def test_steered_scores_overflow_a_naive_softmax():
    """Every A pattern but the equal-scores one sends an fp32 exp(s) softmax without max subtraction to
    Inf / NaN, while the float64 reference is finite with max |ref| >= 0.1 (equal scores: finite, the
    mean of V); and g and a are exact in bf16 (steer_g asserts multiples of 0.5 within 128)."""
    assert torch.tensor(A_STEER).bfloat16().item() == A_STEER
    for what, p, scores, ref in _softmax_inputs():
        assert torch.isfinite(ref).all(), what
        if p != "qzero":
            assert ref.abs().max().item() >= 0.1, what
            assert naive_softmax_nonfinite(scores), what
        else:  # the plain mean of V: ~ N^-1/2, the one pattern a naive softmax survives
            assert ref.abs().max().item() > 0 and not naive_softmax_nonfinite(scores), what


def test_offset_and_equal_scores_references():
    """The offset pattern's reference (taken at g = 0) equals the float64 softmax of the offset scores,
    and q = 0 gives the plain mean of V over the keys."""
    qkv, _, ref, _, _ = mha_case(37, 2, "offset", False)
    assert (E.mha(qkv.double(), 2, MHA_SCALE) - ref).abs().max().item() < 1e-12
    qkv, _, ref, _, _ = mha_case(37, 2, "qzero", False)
    vmean = qkv.double().view(1, 37, 3, 2, 64)[:, :, 2].mean(1, keepdim=True).reshape(1, 1, 128)
    assert (ref - vmean).abs().max().item() < 1e-12


def naive_vs_oracle(shape, groups, kind, bound, bf16):
    """err / tol of fp32 E[x^2] - E[x]^2 moments and of the fp32 oracle on a shifted GroupNorm input
    (act none; bf16: bf16-rounded input, both results rounded to bf16 as the kernel's output is)."""
    x, w, b, pb = gn_case(shape, groups, kind, bf16=bf16)
    x = x.float()
    ref, term, rmax = gn_ref(x, groups, w, b, pb, 1e-5, "none", None)
    tol = bound * rmax.clamp(min=1.0) + term
    n, c = shape[:2]
    pre = (x + pb.view(1, c, 1, 1)).reshape(n, groups, -1)
    mean = pre.mean(-1, keepdim=True)
    var = ((pre * pre).mean(-1, keepdim=True) - mean * mean).clamp(min=0.0)
    naive = ((pre - mean) * torch.rsqrt(var + 1e-5)).reshape(shape) * w.view(1, c, 1, 1) + b.view(1, c, 1, 1)
    oracle = E.group_norm(x, groups, w, b, 1e-5, "none", None, pb)
    if bf16:
        naive, oracle = naive.bfloat16(), oracle.bfloat16()
    return tuple(((t.double() - ref).abs() / tol).max().item() for t in (naive, oracle))


def test_shifted_data_breaks_naive_moments():
    """On the mean >> sigma inputs, fp32 moments taken as E[x^2] - E[x]^2 miss the B tolerance by at
    least 4x, while the fp32 oracle stays within it."""
    for shape, groups, _ in GN_SHAPES:
        for kind in ("shift100", "shift1000"):
            r_naive, r_oracle = naive_vs_oracle(shape, groups, kind, 2e-5, False)
            print(f"moments {shape} {kind}: naive err/tol {r_naive:.1f}, oracle err/tol {r_oracle:.3f}")
            assert r_naive >= 4.0, (shape, kind, r_naive)
            assert r_oracle <= 1.0, (shape, kind, r_oracle)


def test_shifted_data_breaks_naive_moments_bf16():
    """The bf16 form's 8e-3 bound hides naive moments at mean / sigma = 1e2 (printed); the 1e3 input is
    the one that shows them: there they miss the bound on both shapes while the oracle stays within it."""
    for shape, groups in BF16_GN_SHAPES:
        for kind in ("shift100", "shift1000"):
            r_naive, r_oracle = naive_vs_oracle(shape, groups, kind, 8e-3, True)
            print(f"bf16 moments {shape} {kind}: naive err/tol {r_naive:.2f}, oracle err/tol {r_oracle:.3f}")
            assert r_oracle <= 1.0, (shape, kind, r_oracle)
            if kind == "shift1000":
                assert r_naive > 1.0, (shape, kind, r_naive)


@pytest.mark.parametrize("name", list(C_CASES))
def test_ideal_split_meets_the_bars_and_truncation_does_not(name):
    """An ideal bf16x3 emulated in float64 meets both C bars with 2x headroom on every C input; the
    same emulation with a truncated hi (a bias of ~1e-5 of |y| on same-sign data, whatever K) fails
    etf / 8 on the same-sign input where K is long enough: etf falls like K^-1/2 (|randn| products
    weigh like 0.4 K equal terms), below 8e-5 from K ~ 10^3. Every kernel family has such a case
    (TRUNCATION_SHOWS), and those five carry the truncation check; the small-K cases (the two small
    GEMMs, linear_257_128_128, direct_1x1, wino_38_32, wino_16_16) keep the bars on same-sign data but
    would let a truncated split through (printed below: e3 under etf / 8)."""
    op = c_op(name)
    for data in ("same", "scaled"):
        x, w, ref, ref_tf = c_case(name, data)
        e3, etf = c_bars(x3_ideal(op, x, w), ref, ref_tf, data == "scaled")
        print(f"ideal split {name} {data}: e3 {e3.max().item():.3e}, worst e3/etf {(e3 / etf).max().item():.4f}")
        assert (e3 < 1e-5).all() and (e3 <= etf / 16).all(), (name, data)
    x, w, ref, ref_tf = c_case(name, "same")
    e3, etf = c_bars(x3_ideal(op, x, w, truncate=True), ref, ref_tf, False)
    print(f"truncated split {name} same: e3 {e3.item():.3e}, etf/8 {etf.item() / 8:.3e}")
    if name in TRUNCATION_SHOWS:
        assert e3 > etf / 8, (name, e3.item(), etf.item())
