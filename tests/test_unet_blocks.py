"""The refinement U-Net's blocks (model/encoder/matching/ldm_unet.py) against float64 restatements
(oracle/unet_blocks.py), on every route the glue can take and at the shape edges.

Each GPU case runs the real module once under a route census, asserts the C entry points, library
calls and torch.cat calls that ran (the route rules are restated below, `expect_*`), and compares
with the float64 reference at

    bar = FACTOR[class] * (error of the class's CPU emulation on the same case),

both as max-norm errors relative to max |ref|. The emulations (oracle.unet_blocks.Arith): plain
torch fp32; float64 with every convolution an ideal split-bf16 product; torch.autocast("cpu",
bfloat16) with GroupNorm32 semantics. A class is what ran: a few-channel entry -> "few", else a
Winograd entry -> "wino", else "direct"; any bf16x3 entry -> "x3", else "f32"; under autocast "bf16".

Route sets: "direct" (default thresholds: every case is under the direct kernel's FLOP ceiling),
"wino" (_CONV_MAX_FLOP = 0, _WINO_MODE = "all", _FEW off: what the full-size maps take in a
benchmarked step) and "few" (the same with FEW_MIN_PX = 0). Maps with n h w <= 512 stay on the
direct kernel whatever the thresholds, so the attention, downsample and small upsample cases take
the same route in every set; they run in each set all the same.

FACTOR: GPU error / emulation error measured on MI355X for every run of every case (85 runs); the
factor is the smallest power of two >= 2 x the worst ratio of the class (none may need more than 16).

    class         runs  worst ratio  worst case                                    factor
    direct  f32    31   0.89         ResBlock 2x32x0x16x20x32, direct route           2
    wino    f32    11   1.24         ResBlock 2x128x128x16x20x128, production         4
    direct  x3     11   1.00         AttentionBlock 4x64x5x7x2 (0.9989)               2
    wino    x3     11   2.18         ResBlock 2x32x0x16x20x64, production             8
    few     x3      4   1.04         ResBlock 2x32x0x16x20x32, few-channel            4
    bf16           16   1.37         Upsample 2x32x5x7 (the library's bf16 conv)      4

(The split-bf16 Winograd kernel splits the transformed tiles V = B^T d B and filters G g G^T
(csrc/winoconv3.hip), not the operands, and its output transform adds 9 of the 16 products per pixel:
about twice the ideal split of the direct product, a constant.)

bf16 autocast: tsplat_conv2d_bf16_fwd takes a convolved width that is a multiple of 8. None of the
ResBlock / Upsample shapes above has one (20, 15, 19, 14 and 20 wide), so all of them assert the
fallback (the library's bf16 convolution); the *_BF16_EXTRA shapes (24 wide) and the attention
blocks with t = 24 and 48 assert the HIP kernel; t = 35 asserts the fallback.

The CPU tests (unmarked) check the restatements against the module glue run on the oracle ops, bound
the emulation errors, and show that every case separates its mutants (oracle.unet_blocks.MUTANTS)
from the reference by >= 10 x the loosest bar it is checked against. GroupNorm4 "run as 8 groups"
cannot be stated for 36 channels (36 % 8 != 0); its mutant runs the 8-group kernel's 36 // 8 = 4
channels per group, 9 groups.
"""
import copy
import functools
import sys
from collections import Counter
from contextlib import contextmanager
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
from canonical import canonical_init, seeded  # noqa: E402

from oracle import encoder_ops as E  # noqa: E402
from oracle import unet_blocks as U  # noqa: E402

FACTOR = {("direct", "f32"): 2, ("wino", "f32"): 4, ("direct", "x3"): 2, ("wino", "x3"): 8, ("few", "x3"): 4, "bf16": 4}

# ResBlock (n, c1, c2, h, w, cout); AttentionBlock (vb, c, h, w, views); Downsample / Upsample (n, c, h, w)
RES = [(2, 32, 0, 16, 20, 32), (3, 32, 0, 13, 15, 32), (2, 32, 0, 16, 20, 64), (2, 32, 0, 17, 19, 36),
       (2, 32, 32, 16, 20, 32), (2, 64, 32, 17, 19, 32), (2, 128, 128, 16, 20, 128), (2, 16, 16, 16, 20, 32)]
RES_FEW = [RES[0], RES[4], RES[7]]  # w % 4 == 0, ci <= 64, co <= 32
RES_BF16_EXTRA = [(2, 32, 32, 12, 24, 32), (2, 32, 0, 12, 24, 36)]  # w % 8 == 0: the bf16 HIP kernel
ATT = [(4, 64, 5, 7, 2), (6, 32, 4, 6, 3), (3, 128, 6, 8, 1)]
DOWN = [(2, 32, 9, 13), (2, 128, 8, 12)]
UP = [(2, 32, 5, 7), (2, 128, 8, 10)]
UP_BF16_EXTRA = [(2, 32, 6, 12)]
UNET = (4, 32, 18, 20)  # (v b) = (2 2); 18 x 20 and 9 x 10 maps; 64 + 32 concat parts
FP32_CASES = ([("res", g) for g in RES] + [("att", g) for g in ATT] + [("down", g) for g in DOWN]
              + [("up", g) for g in UP] + [("unet", UNET)])
BF16_CASES = ([("res", g) for g in RES + RES_BF16_EXTRA] + [("att", g) for g in ATT]
              + [("up", g) for g in UP + UP_BF16_EXTRA])
ALL_CASES = FP32_CASES + [c for c in BF16_CASES if c not in FP32_CASES]
_id = lambda case: case[0] + "-" + "x".join(map(str, case[1]))

# Parameters: canonical weights (randn / sqrt(fan_in)), conv biases randn, norm weights 1 + 0.5 randn,
# norm biases 0.2 randn; inputs randn. The loosest bar of most cases is the bf16 one, ~2.5e-2 of
# max |ref|, so a mutant has to move the output by a quarter of its range. Of seeds 7000 .. 7047, each
# case takes the one whose weakest mutant lies furthest from the reference (>= 20 x the loosest bar).
CONV_BIAS = 1.0
SEEDS = {("res", RES[0]): 7024, ("res", RES[1]): 7020, ("res", RES[2]): 7023, ("res", RES[3]): 7038,
         ("res", RES[4]): 7028, ("res", RES[5]): 7002, ("res", RES[6]): 7022, ("res", RES[7]): 7018,
         ("res", RES_BF16_EXTRA[0]): 7020, ("res", RES_BF16_EXTRA[1]): 7044,
         ("att", ATT[0]): 7040, ("att", ATT[1]): 7023, ("att", ATT[2]): 7019,
         ("up", UP[0]): 7000, ("up", UP[1]): 7046, ("up", UP_BF16_EXTRA[0]): 7036,
         ("down", DOWN[0]): 7011, ("down", DOWN[1]): 7012, ("unet", UNET): 7015}


# ===================================================================== modules, references, emulations
def _init(m, seed: int):
    canonical_init(m, seed)
    with torch.no_grad():
        for i, mod in enumerate(m.modules()):
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.copy_(1 + 0.5 * seeded(mod.weight.shape, seed * 1000 + 2 * i))
                mod.bias.copy_(0.2 * seeded(mod.bias.shape, seed * 1000 + 2 * i + 1))
            elif isinstance(mod, (torch.nn.Conv1d, torch.nn.Conv2d)):
                mod.bias.copy_(CONV_BIAS * seeded(mod.bias.shape, seed * 1000 + 2 * i))
    return m.eval()


@functools.lru_cache(maxsize=None)
def build(kind: str, geo):
    """(module on the CPU, inputs); never modified: the GPU tests run a deep copy."""
    from transplat_amd.model.encoder.matching import ldm_unet as L

    seed = SEEDS[(kind, geo)]
    if kind == "res":
        n, c1, c2, h, w, co = geo
        m = L.ResBlock(c1 + c2, out_channels=co)
        xs = (seeded((n, c1, h, w), seed), seeded((n, c2, h, w), seed + 500) if c2 else None)
    elif kind == "att":
        vb, c, h, w, views = geo
        m = L.AttentionBlock(c, num_head_channels=32, num_frames=views, use_cross_view_self_attn=views > 1)
        xs = (seeded((vb, c, h, w), seed),)
    elif kind in ("down", "up"):
        m = (L.Downsample if kind == "down" else L.Upsample)(geo[1], out_channels=geo[1])
        xs = (seeded(geo, seed),)
    else:
        m = L.UNetModel(image_size=None, in_channels=32, model_channels=32, out_channels=32, num_res_blocks=1,
                        attention_resolutions=(2,), channel_mult=(1, 2), num_head_channels=32, dims=2, postnorm=True,
                        num_frames=2, use_cross_view_self_attn=True)
        xs = (seeded(geo, seed),)
    return _init(m, seed), xs


_RESTATE = {"res": U.res_block, "att": U.attention_block, "down": U.downsample, "up": U.upsample, "unet": U.unet}


def restate(kind, geo, arith: str = "f64", mut=frozenset()):
    m, xs = build(kind, geo)
    with torch.no_grad():
        return _RESTATE[kind](m, *xs, ar=U.Arith(arith), mut=frozenset(mut))


@functools.lru_cache(maxsize=None)
def reference(kind, geo):
    return restate(kind, geo)


@functools.lru_cache(maxsize=None)
def emu_err(kind, geo, arith: str) -> float:
    """Error of the arithmetic class's CPU emulation against the float64 reference."""
    return U.rel_err(restate(kind, geo, arith), reference(kind, geo))


def mutants_of(kind, geo):
    if kind == "res":
        return (["no_bias1", "no_bias2"] + (["concat_swap", "skip_x_only"] if geo[2] else [])
                + (["gn_groups"] if geo[5] % 8 else []))
    if kind == "att":
        return ["no_proj_bias"] + (["vb_as_bv", "no_fold"] if geo[4] > 1 else [])
    if kind == "down":
        return ["stride_offset"]
    if kind == "up":
        return ["zero_insert"]
    return [m for m in U.MUTANTS if m != "gn_groups"]  # the U-Net has no 4-group norm


# ===================================================================== the route rules, restated
F32_DIRECT, X3_DIRECT = "tsplat_conv2d_f32_zsplit_fwd", "tsplat_conv2d_bf16x3_fwd"
F32_WINO, X3_WINO, X3_FEW = ("tsplat_conv3x3_wino_cat_f32_fwd", "tsplat_conv3x3_wino_bf16x3_ex_fwd",
                             "tsplat_conv3x3_few_bf16x3_fwd")
BF16_CONV, GN_BF16, ATTN = "tsplat_conv2d_bf16_fwd", "tsplat_group_norm_bf16_fwd", "tsplat_qkv_attention_cf_fwd"
GN, GN_CAT = "tsplat_group_norm_fwd", "tsplat_group_norm_cat_res_fwd"
GEMM = "baddbmm"  # the full-resolution 1x1 as one batched library GEMM


class Expect:
    def __init__(self):
        self.names, self.cats, self.gemms, self.libconvs = Counter(), 0, 0, 0

    def conv(self, entry):
        if entry == GEMM:
            self.gemms += 1
        else:
            self.names[entry] += 1

    def route(self, autocast: bool):
        """The arithmetic class of what is expected to run (see the module docstring)."""
        if autocast:
            return "bf16"
        names = list(self.names)
        route = "few" if X3_FEW in names else "wino" if any("wino" in n for n in names) else "direct"
        return route, "x3" if any("bf16x3" in n for n in names) else "f32"


def _wino(rs, dense, ci, co, w):
    if dense == "fp32":
        return F32_WINO
    return X3_FEW if rs == "few" and co <= 32 and ci <= 64 and w % 4 == 0 else X3_WINO


def _conv(rs, dense, k, npx, ci, co, w, two_src=False):
    """The entry point of one convolution outside autocast: npx = n h w of the (strided) output map."""
    flop = 2.0 * npx * co * ci * k * k
    assert flop <= 1.5e9, "every case sits under the direct kernel's default FLOP ceiling"
    if rs == "direct" or npx <= 512:
        return X3_DIRECT if dense == "bf16x3" and (k == 1 or (ci >= 64 and flop >= 0.5e9)) else F32_DIRECT
    if k == 3:
        return _wino(rs, dense, ci, co, w)
    return X3_DIRECT if dense == "bf16x3" and two_src else GEMM  # the concat-free block forces the direct 1x1


def expect_res(geo, rs, dense, autocast, e=None):
    n, c1, c2, h, w, co = geo
    e = e or Expect()
    ci, npx, skipconv = c1 + c2, n * h * w, co != c1 + c2
    if autocast:
        if w % 8 == 0:
            e.names[BF16_CONV] += 2 + skipconv
        else:
            e.libconvs += 2 + skipconv
        e.names[GN_BF16] += 2
        e.cats += bool(c2)
        return e
    first = _conv(rs, dense, 3, npx, ci, co, w)
    e.conv(first)
    e.conv(_conv(rs, dense, 3, npx, co, co, w))
    # cat([x, x2]) is read in place by the direct kernel, and by the concat-free block of the bf16x3 mode
    in_place = bool(c2) and (first in (F32_DIRECT, X3_DIRECT) or dense == "bf16x3")
    e.cats += bool(c2) and not in_place
    if skipconv:
        e.conv(_conv(rs, dense, 1, npx, ci, co, w, two_src=in_place))
    e.names[GN] += 1
    e.names[GN_CAT if in_place and not skipconv else GN] += 1  # the pair residual
    return e


def expect_att(geo, rs, dense, autocast, e=None):
    vb, c, h, w, views = geo
    e = e or Expect()
    t = h * w
    if autocast:
        if t % 8 == 0:
            e.names[BF16_CONV] += 2
        else:
            e.libconvs += 2
        e.names[GN_BF16] += 1
    else:
        assert vb * t <= 512, "the Conv1d projections stay on the direct kernel only on maps this small"
        for _ in range(2):
            e.conv(_conv(rs, dense, 1, vb * t, c, c, 1))
        e.names[GN] += 1
    e.names[ATTN] += 1
    return e


def expect_down(geo, rs, dense, autocast=False, e=None):
    n, c, h, w = geo
    e = e or Expect()
    e.conv(_conv(rs, dense, 3, n * (h // 2) * (w // 2), c, c, w))
    return e


def expect_up(geo, rs, dense, autocast, e=None):
    n, c, h, w = geo
    e = e or Expect()
    if autocast:
        if (2 * w) % 8 == 0:
            e.names[BF16_CONV] += 1
        else:
            e.libconvs += 1
    else:
        e.conv(_conv(rs, dense, 3, n * 2 * h * 2 * w, c, c, 2 * w))
    return e


def expect_unet(geo, rs, dense, autocast=False):
    """The census of the whole model, block by block as UNetModel.forward visits them."""
    m, _ = build("unet", geo)
    n, c, h, w = geo
    e = Expect()

    def step(mod, c, h, w, c2=0):
        kind = type(mod).__name__
        if kind == "ResBlock":
            expect_res((n, c, c2, h, w, mod.out_channels), rs, dense, False, e)
            return mod.out_channels, h, w
        if kind == "AttentionBlock":
            expect_att((n, c, h, w, 2), rs, dense, False, e)
        elif kind == "Downsample":
            expect_down((n, c, h, w), rs, dense, False, e)
            return c, (h + 1) // 2, (w + 1) // 2
        elif kind == "Upsample":
            expect_up((n, c, h, w), rs, dense, False, e)
            return c, 2 * h, 2 * w
        elif kind == "Conv2d":  # the stem, through install_conv2d_dispatch: Winograd before the direct kernel
            e.conv(_wino(rs, dense, c, mod.out_channels, w))
            return mod.out_channels, h, w
        return c, h, w

    hs = []
    for block in m.input_blocks:
        for mod in block:
            c, h, w = step(mod, c, h, w)
        hs.append(c)
    for mod in m.middle_block:
        c, h, w = step(mod, c, h, w)
    for block in m.output_blocks:
        mods = list(block)
        c, h, w = step(mods[0], c, h, w, c2=hs.pop())
        for mod in mods[1:]:
            c, h, w = step(mod, c, h, w)
    e.conv(_conv(rs, dense, 3, n * h * w, c, m.out[0].out_channels, w))
    e.names[GN] += 1
    return e


_EXPECT = {"res": expect_res, "att": expect_att, "down": expect_down, "up": expect_up, "unet": expect_unet}


def expect(kind, geo, rs, dense, autocast=False) -> Expect:
    return _EXPECT[kind](geo, rs, dense, autocast)


def runs_of(kind, geo):
    """Every (route set, dense mode, autocast) the GPU tests run this case in."""
    runs = []
    if (kind, geo) in FP32_CASES:
        runs += [(rs, dense, False) for rs in ("direct", "wino") for dense in ("fp32", "bf16x3")]
        if (kind == "res" and geo in RES_FEW) or kind == "unet":
            runs.append(("few", "bf16x3", False))
    if (kind, geo) in BF16_CASES:
        runs.append(("direct", "fp32", True))
    return runs


def bar_of(kind, geo, rs, dense, autocast):
    """(class, emulation error, bar) of one run."""
    cls = expect(kind, geo, rs, dense, autocast).route(autocast)
    emu = emu_err(kind, geo, "bf16" if autocast else cls[1])
    return cls, emu, FACTOR[cls] * emu


# ===================================================================== CPU: the cases detect what they claim
@pytest.fixture
def cpu_ops(monkeypatch):
    from transplat_amd import kernels

    for name in E.KERNEL_RESTATEMENTS:
        monkeypatch.setattr(kernels, name, getattr(E, name))


@pytest.mark.parametrize("case", FP32_CASES, ids=_id)
def test_reference_matches_the_module_glue(cpu_ops, case):
    """The float64 restatement against the module's own forward run on the fp32 oracle ops (the glue
    with every convolution on the oracle's direct form): two independent statements of the block agree to
    1e-5 of max |ref|, the fp32 class (the emulations come to ~3e-7) with room for another summation
    order, and 10^3 below the smallest mutant."""
    m, xs = build(*case)
    with torch.no_grad():
        out = m(*xs)
    err = U.rel_err(out, reference(*case))
    print(f"[unet blocks] {_id(case)}: glue on oracle ops vs float64 {err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("case", ALL_CASES, ids=_id)
def test_emulation_errors(case):
    """The bars' ingredients, within what the formats allow. fp32: unit roundoff 6e-8 per operation,
    adding like a random walk through two convolutions and two norms (a block: ~3e-7) or the ~50 layers of
    the whole model (~1e-6): under 5e-6. Ideal bf16x3: 3 x 2^-18 = 1.1e-5 per product (kernels.py,
    _DENSE), averaged over the reduction (a block: ~5e-6, the model ~2e-5): above the fp32 figure and
    under 1e-4. bf16: one rounding of the output alone is up to 2^-9 = 2e-3 of max |ref|, a block rounds
    four to six times: between 5e-4 and 5e-2."""
    errs = {a: emu_err(*case, a) for a in ("f32", "x3")}
    if case in BF16_CASES:
        errs["bf16"] = emu_err(*case, "bf16")
    print(f"[unet blocks] {_id(case)}: emulation errors " + "  ".join(f"{a} {v:.3e}" for a, v in errs.items()))
    assert 0 < errs["f32"] < 5e-6
    assert errs["f32"] < errs["x3"] < 1e-4
    if "bf16" in errs:
        assert 5e-4 < errs["bf16"] < 5e-2


@pytest.mark.parametrize("case", ALL_CASES, ids=_id)
def test_cases_separate_their_mutants(case):
    """Every mutant of the float64 reference lies >= 10 x the loosest bar of the case away from it."""
    loosest = max(bar_of(*case, *run)[2] for run in runs_of(*case))
    ref = reference(*case)
    muts = mutants_of(*case)
    assert muts
    for mut in muts:
        d = U.rel_err(restate(*case, mut=(mut,)), ref)
        print(f"[unet blocks] {_id(case)}: mutant {mut} {d:.3e}  (10 x loosest bar {10 * loosest:.3e})")
        assert d >= 10 * loosest, (mut, d, loosest)


def test_route_rules_reach_what_the_cases_claim():
    """The restated rules send the cases where the header says: every class has a case, the concat-free
    block (two-source Winograd / few-channel launch, forced two-source 1x1, pair residual) and both
    autocast routes are expected somewhere."""
    classes = {bar_of(*case, *run)[0] for case in ALL_CASES for run in runs_of(*case)}
    assert classes == set(FACTOR)
    e = expect("res", RES[4], "wino", "bf16x3")
    assert (e.names[X3_WINO], e.names[X3_DIRECT], e.cats, e.gemms) == (2, 1, 0, 0)
    e = expect("res", RES[7], "few", "bf16x3")
    assert (e.names[X3_FEW], e.names[GN_CAT], e.cats) == (2, 1, 0)
    assert expect("res", RES[4], "wino", "fp32").names == Counter({F32_WINO: 2, GN: 2})
    assert expect("res", RES[1], "direct", "fp32", True).libconvs == 2
    assert expect("res", RES_BF16_EXTRA[0], "direct", "fp32", True).names[BF16_CONV] == 3
    assert expect("att", ATT[0], "direct", "fp32", True).libconvs == 2


# ===================================================================== GPU
@contextmanager
def census():
    """routes.record() plus the name of every C entry point that returned."""
    from transplat_amd import _lib, routes

    names = []
    with routes.record() as r:
        inner = _lib.ROUTE_HOOK

        def hook(what, route=None):
            names.append(what)
            inner(what, route)

        _lib.ROUTE_HOOK = hook
        try:
            yield r, names
        finally:
            _lib.ROUTE_HOOK = inner


def pin(monkeypatch, rs):
    from transplat_amd import kernels as K

    if rs != "direct":
        monkeypatch.setattr(K, "_CONV_MAX_FLOP", 0.0)
        monkeypatch.setattr(K, "_WINO_MODE", "all")
        if rs == "few":
            monkeypatch.setattr(K, "FEW_MIN_PX", 0)
        else:
            monkeypatch.setattr(K, "_FEW", False)


def run_case(device, monkeypatch, case, rs, dense, autocast=False):
    from transplat_amd import kernels as K
    from transplat_amd import routes

    kind, geo = case
    m, xs = build(kind, geo)
    exp = expect(kind, geo, rs, dense, autocast)
    cls, emu, bar = bar_of(kind, geo, rs, dense, autocast)
    md = copy.deepcopy(m).to(device)
    if kind == "unet":
        K.install_conv2d_dispatch(md)  # as EncoderTrans does: the stem is a plain Conv2d
    xd = [t.to(device) if t is not None else None for t in xs]
    pin(monkeypatch, rs)
    cats, real_cat = [], torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **k: (cats.append(1), real_cat(*a, **k))[1])
    with torch.no_grad(), K.dense_precision(dense), torch.autocast("cuda", torch.bfloat16, enabled=autocast):
        with census() as (r, names):
            y = md(*xd)
    monkeypatch.undo()
    out = y.float().cpu()
    got = Counter(n for n in names if n in routes._HIP)
    libconvs = [x for x in r.library if x[0] not in routes._GEMMS]
    gemms = [x for x in r.library if x[0] in routes._GEMMS]
    tag = f"{_id(case)} {rs} {dense}{' autocast' if autocast else ''}"
    print(f"[unet blocks] {tag}: ran {dict(got)}, {len(gemms)} library GEMMs, {len(libconvs)} library convs, "
          f"{len(cats)} torch.cat")
    assert got == exp.names, (tag, dict(got), dict(exp.names))
    assert len(cats) == exp.cats, (tag, len(cats), exp.cats)
    assert [g[0] for g in gemms] == [GEMM] * exp.gemms, (tag, gemms)
    assert len(libconvs) == exp.libconvs, (tag, libconvs)
    if not autocast:
        assert "library convs (MIOpen)" not in r.by_category(), (tag, r.library)
    err = U.rel_err(out, reference(kind, geo))
    print(f"[unet blocks] {tag}: class {cls}  max error {err:.3e} of max |ref|  emulation {emu:.3e}  "
          f"ratio {err / emu:.2f}  (bar {bar:.3e} = {FACTOR[cls]} x emulation)")
    assert err < bar, f"{tag}: max error {err:.3e}, bar {bar:.3e} ({FACTOR[cls]} x {emu:.3e})"


DENSE = ["fp32", "bf16x3"]
ROUTE_SETS = ["direct", "wino"]


@pytest.mark.gpu
@pytest.mark.parametrize("dense", DENSE)
@pytest.mark.parametrize("rs", ROUTE_SETS)
@pytest.mark.parametrize("geo", RES, ids=lambda g: "x".join(map(str, g)))
def test_res_block(device, monkeypatch, geo, rs, dense):
    run_case(device, monkeypatch, ("res", geo), rs, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", RES_FEW, ids=lambda g: "x".join(map(str, g)))
def test_res_block_few_channel(device, monkeypatch, geo):
    """tsplat_conv3x3_few_bf16x3_fwd for both 3x3s; with x2 as a two-source launch (no torch.cat), the
    1x1 skip forced onto the two-source direct kernel, an identity skip as the pair residual."""
    run_case(device, monkeypatch, ("res", geo), "few", "bf16x3")


@pytest.mark.gpu
@pytest.mark.parametrize("dense", DENSE)
@pytest.mark.parametrize("rs", ROUTE_SETS)
@pytest.mark.parametrize("geo", ATT, ids=lambda g: "x".join(map(str, g)))
def test_attention_block(device, monkeypatch, geo, rs, dense):
    run_case(device, monkeypatch, ("att", geo), rs, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("dense", DENSE)
@pytest.mark.parametrize("rs", ROUTE_SETS)
@pytest.mark.parametrize("kind,geo", [("down", g) for g in DOWN] + [("up", g) for g in UP], ids=lambda v: str(v))
def test_resample(device, monkeypatch, kind, geo, rs, dense):
    run_case(device, monkeypatch, (kind, geo), rs, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("rs,dense", [(rs, d) for rs in ROUTE_SETS for d in DENSE] + [("few", "bf16x3")])
def test_unet_two_scenes(device, monkeypatch, rs, dense):
    """The whole model on (v b) = (2 2) scenes against the composed float64 reference."""
    run_case(device, monkeypatch, ("unet", UNET), rs, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("case", BF16_CASES, ids=_id)
def test_bf16_autocast(device, monkeypatch, case):
    """Config C3's convolutions: tsplat_conv2d_bf16_fwd + tsplat_group_norm_bf16_fwd and no library
    convolution where the convolved width is a multiple of 8, the library's bf16 convolution where not."""
    run_case(device, monkeypatch, case, "direct", "fp32", autocast=True)
