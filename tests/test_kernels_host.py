"""Host-side pieces of transplat_amd.kernels that need no GPU: the one derived-tensor cache, the
packed weight layouts, conv2d_fallback's argument normalisation and the convolution launch shapes."""
import gc

import pytest
import torch
import torch.nn.functional as F

from transplat_amd import kernels as K

CACHED = [K.conv_pack_weight, K.conv_pack_weight_x3, K.conv_bf16_pack_weight, K._bf16_rounded_bias]
CACHE_SHAPES = [(40, 6, 3, 3), (8, 4, 1, 1)]


def _weight(shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture
def fresh_cache(monkeypatch):
    monkeypatch.setattr(K, "_DERIVED", {})
    return K._DERIVED


@pytest.mark.parametrize("shape", CACHE_SHAPES)
@pytest.mark.parametrize("fn", CACHED, ids=lambda f: f.__name__)
def test_cache_hit_and_version(fn, shape, fresh_cache):
    w = _weight(shape)
    first = fn(w)
    assert fn(w) is first
    assert len(fresh_cache) == 1
    w.add_(1)
    second = fn(w)
    assert second is not first
    assert fn(w) is second
    assert len(fresh_cache) == 1
    assert torch.equal(second, fn(w.clone()))  # the new version's value, not the stale one
    assert not torch.equal(second.float(), first.float())


@pytest.mark.parametrize("shape", CACHE_SHAPES)
def test_cache_tags_coexist(shape, fresh_cache):
    w = _weight(shape)
    got = [fn(w) for fn in CACHED]
    assert len(fresh_cache) == len(CACHED)
    assert all(key[0] == id(w) for key in fresh_cache)
    for fn, first in zip(CACHED, got):
        assert fn(w) is first  # no tag evicted another
    assert len(fresh_cache) == len(CACHED)


@pytest.mark.parametrize("shape", CACHE_SHAPES)
@pytest.mark.parametrize("fn", CACHED, ids=lambda f: f.__name__)
def test_cache_prunes_dead_entries(fn, shape, fresh_cache):
    w = _weight(shape)
    fn(w)
    (ref, _, _), = fresh_cache.values()
    del w
    gc.collect()
    assert ref() is None and len(fresh_cache) == 1  # dead, but kept until the dict passes its bound
    others = [torch.zeros(2) for _ in range(K._DERIVED_MAX + 2)]
    for t in others:
        K._bf16_rounded_bias(t)
    assert all(v[0] is not ref and v[0]() is not None for v in fresh_cache.values())
    assert len(fresh_cache) == len(others)


# The layouts below restate the pack functions' docstrings index by index (plain Python loops over
# nested lists), independently of the reshape / permute chains under test.
LAYOUT_SHAPES = [(40, 18, 3, 3), (32, 16, 1, 1), (8, 4, 1)]


def _taps(w):
    co, ci = w.shape[:2]
    return w.reshape(co, ci, -1)


def _at(rows, o, i, tap):
    return rows[o][i][tap] if o < len(rows) and i < len(rows[0]) else 0.0


@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_conv_pack_weight_layout(shape):
    """[ceil(cout / 32), k * k, cin / 2, 2, 32]: entry [b, tap, p, e, m] = w[32 b + m][2 p + e][tap]."""
    w = _weight(shape, 1)
    rows = _taps(w).tolist()
    co, ci, taps = len(rows), len(rows[0]), len(rows[0][0])
    want = [[[[[_at(rows, 32 * b + m, 2 * p + e, tap) for m in range(32)] for e in range(2)]
              for p in range(ci // 2)] for tap in range(taps)] for b in range((co + 31) // 32)]
    got = K.conv_pack_weight(w)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, torch.tensor(want, dtype=torch.float32))


@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_conv_pack_weight_x3_layout(shape):
    """[ceil(cout / 32)][k * k][ceil(cin / 16)][hi, lo][64 lanes][8]: lane l, element j =
    cout 32 b + (l & 31), cin 16 g + 8 (l >> 5) + j; hi = bf16(w), lo = bf16(w - hi); zero-padded."""
    w = _weight(shape, 2)
    hi = _taps(w).bfloat16()
    lo = (_taps(w) - hi.float()).bfloat16()
    co, ci, taps = hi.shape
    parts = (hi.float().tolist(), lo.float().tolist())
    want = [[[[[[_at(part, 32 * b + (l & 31), 16 * g + 8 * (l >> 5) + j, tap) for j in range(8)] for l in range(64)]
               for part in parts] for g in range((ci + 15) // 16)] for tap in range(taps)]
            for b in range((co + 31) // 32)]
    got = K.conv_pack_weight_x3(w)
    assert got.dtype == torch.bfloat16 and got.is_contiguous()
    want = torch.tensor(want, dtype=torch.bfloat16)
    assert got.numel() == want.numel()
    assert torch.equal(got.reshape(want.shape), want)


@pytest.mark.parametrize("shape", LAYOUT_SHAPES)
def test_conv_bf16_pack_weight_layout(shape):
    """[ceil(cout / 32)][ceil(cin / 16)][k * k][64 lanes][8]: lane c + 32 h, element e =
    bf16(w[32 b + c][16 j + 8 h + e][tap]); zero-padded."""
    w = _weight(shape, 3)
    rows = _taps(w).bfloat16().float().tolist()
    co, ci, taps = len(rows), len(rows[0]), len(rows[0][0])
    want = [[[[[_at(rows, 32 * b + (l & 31), 16 * j + 8 * (l >> 5) + e, tap) for e in range(8)] for l in range(64)]
              for tap in range(taps)] for j in range((ci + 15) // 16)] for b in range((co + 31) // 32)]
    got = K.conv_bf16_pack_weight(w)
    assert got.dtype == torch.bfloat16 and got.is_contiguous()
    want = torch.tensor(want, dtype=torch.bfloat16)
    assert got.numel() == want.numel()
    assert torch.equal(got.reshape(want.shape), want)


def test_square():
    assert [K._square(v) for v in (3, (2, 2), [1, 1], (0, 0))] == [3, 2, 1, 0]
    assert [K._square(v) for v in ((1, 2), "same", (1, 1, 2))] == [-1, -1, -1]


@pytest.mark.parametrize("dilation", [1, (1, 1), 2, (2, 2)])
def test_conv2d_fallback_dilation(dilation, monkeypatch):
    """An int or a pair dilation; the call is described once, only dilation 1 is offered to the bf16x3
    kernels (asked as if on the device in that mode), and on host tensors every case is F.conv2d."""
    asked = []
    real = K.conv_route
    monkeypatch.setattr(K, "conv_route", lambda call, *a, **k: asked.append(call) or real(call, *a, **k))
    x, w, b = _weight((2, 4, 9, 11), 4), _weight((6, 4, 3, 3), 5), _weight((6,), 6)
    got = K.conv2d_fallback(x, w, b, 1, 2, dilation, 1)
    assert torch.equal(got, F.conv2d(x, w, b, 1, 2, dilation, 1))
    assert len(asked) == 1 and asked[0].dilation == (1 if dilation in (1, (1, 1)) else 2)
    offered = [real(K.conv_call(w, (x,), 1, pad, dilation, on_gpu=True, dense="bf16x3"), K.SITE_LIBFREE) for pad in (1, 2)]
    assert offered == (["wino_joined", None] if dilation in (1, (1, 1)) else [None, None])


# (ksplit, zsplit) per _ZSPLIT in (-1, 0, 2), by case: literals from a run of the loops of the commit
# before the shared helpers (conv2d_direct, conv_zsplit, _conv2d_direct_x3, conv2d_nhwc as they stood,
# default knobs), not from the helpers under test.
ZSPLITS = (-1, 0, 2)
DIRECT_3X3 = {(1, 1): [(1, 1), (1, 1), (1, 1)], (4, 128): [(16, 8), (16, 1), (16, 2)],
              (512, 16): [(8, 1), (8, 1), (8, 1)], (513, 16): [(8, 1), (8, 1), (8, 1)],
              (8192, 64): [(1, 1), (1, 1), (1, 1)]}
DIRECT_1X1 = {(1, 4): [(1, 1), (1, 1), (1, 1)], (2048, 64): [(8, 1), (8, 1), (8, 1)],
              (2049, 64): [(4, 1), (4, 1), (4, 1)]}
NHWC = {(8, 384): [16, 16], (4096, 2): [1, 1]}  # ksplit for k = 3, 1
X3 = {(1, 9): [(8, 1), (8, 1), (8, 1)], (8, 432): [(16, 8), (16, 1), (16, 2)],
      (256, 16): [(16, 1), (16, 1), (16, 1)]}


@pytest.fixture
def default_shape_knobs(monkeypatch):
    for name, value in (("_CONV3_WAVES", 8192), ("_CONV3_PAIRS", 2), ("_CONV1_WAVES", 16384), ("_CONV1_PAIRS", 8),
                        ("_ZSPLIT_WGS", 256), ("_ZSPLIT_MIN", 1)):
        monkeypatch.setattr(K, name, value)


def _direct_shape(tiles, pairs, k):
    # conv2d_direct's launch shape
    cap, min_pairs = (K._CONV3_WAVES, K._CONV3_PAIRS) if k == 3 else (K._CONV1_WAVES, K._CONV1_PAIRS)
    ksplit = K._wave_split(tiles, pairs, cap, min_pairs)
    return ksplit, K.conv_zsplit(tiles, pairs, ksplit, k) if ksplit == 16 else 1


@pytest.mark.parametrize("zi", range(3))
def test_launch_shapes_match_previous_loops(zi, monkeypatch, default_shape_knobs):
    monkeypatch.setattr(K, "_ZSPLIT", ZSPLITS[zi])
    for k, table in ((3, DIRECT_3X3), (1, DIRECT_1X1)):
        for (tiles, pairs), want in table.items():
            assert _direct_shape(tiles, pairs, k) == want[zi], (k, tiles, pairs)
    for (tiles, units), want in X3.items():
        assert K._conv_x3_shape(tiles, units) == want[zi], (tiles, units)
    for (tiles, pairs), want in NHWC.items():
        assert [K._wave_split(tiles, pairs, 4096, 2), K._wave_split(tiles, pairs, 4096, 16)] == want


# ---- window attention: the launch plan through its C entry points (the library loads without a GPU)
WINATTN_SHAPES = {  # (b, h, w, key views, splits) -> key split of the exact-fp32 128-query kernel
    (1, 64, 64, 1, 2): 8,
    (2, 64, 64, 1, 2): 4,
    (8, 64, 64, 1, 2): 1,
    (1, 96, 128, 2, 2): 4,
    (1, 32, 96, 1, 2): 4,
    (2, 16, 16, 1, 2): 0,  # L = 64: another kernel serves it
}
WINATTN_KNOBS = ("TSPLAT_WINATTN", "TSPLAT_WINATTN_KSPLIT", "TSPLAT_WINATTN_BF16", "TSPLAT_WINATTN_X3",
                 "TSPLAT_WINATTN_X3_PRIO", "TSPLAT_WINATTN_X3_XCD")


def _choose_ksplit(base, key_tiles, target):
    ks = 1
    while base * ks < target and ks * 2 <= key_tiles and key_tiles % (ks * 2) == 0 and ks < 8:
        ks *= 2
    return ks


def _winattn_bytes(shape, ks):
    b, h, w, m, s = shape
    return b * s * s * ks * (h // s) * (w // s) * 130 * 4 if ks > 1 else 0


@pytest.fixture
def winattn_lib(monkeypatch):
    from transplat_amd import _lib
    for name in WINATTN_KNOBS:
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


@pytest.mark.parametrize("shape", WINATTN_SHAPES)
def test_win_attn_split_and_workspace_agree(shape, winattn_lib, monkeypatch):
    lib = winattn_lib
    b, h, w, m, s = shape
    L = (h // s) * (w // s)
    tiles = L * m // 64
    ks = WINATTN_SHAPES[shape]
    assert lib.tsplat_win_attn_split(*shape) == ks
    assert ks == (_choose_ksplit(L // 128 * s * s * b, tiles, 256) if L % 128 == 0 else 0)
    # L = 64 runs the 64-query kernel: its own split (two workgroups per CU), never reported by _split
    ks_ws = ks if ks else _choose_ksplit(L // 64 * s * s * b, tiles, 512)
    assert lib.tsplat_win_attn_workspace_bytes(*shape) == _winattn_bytes(shape, ks_ws)
    assert K._win_attn_workspace_bytes(lib, "x3", *shape) == K._win_attn_workspace_bytes(lib, "fp32", *shape)
    bf16_bytes = lib.tsplat_win_attn_bf16_workspace_bytes(*shape)
    assert bf16_bytes == (_winattn_bytes(shape, _choose_ksplit(L // 128 * s * s * b, tiles, 512)) if L % 128 == 0 else 0)

    monkeypatch.setenv("TSPLAT_WINATTN_KSPLIT", "2")
    forced = 2 if tiles % 2 == 0 else None
    assert lib.tsplat_win_attn_split(*shape) == ((forced or ks) if L % 128 == 0 else 0)
    assert lib.tsplat_win_attn_workspace_bytes(*shape) == _winattn_bytes(shape, forced or ks_ws)
    assert K._win_attn_workspace_bytes(lib, "x3", *shape) == K._win_attn_workspace_bytes(lib, "fp32", *shape)
    assert lib.tsplat_win_attn_bf16_workspace_bytes(*shape) == bf16_bytes  # the bf16 family has no forced split
    monkeypatch.delenv("TSPLAT_WINATTN_KSPLIT")

    monkeypatch.setenv("TSPLAT_WINATTN", "16")
    assert lib.tsplat_win_attn_split(*shape) == 0  # 0 whenever the knob is set at all
    ks16 = _choose_ksplit(L // 64 * s * s * b, tiles, 512)  # the 64-query rule
    assert lib.tsplat_win_attn_workspace_bytes(*shape) == _winattn_bytes(shape, ks16)
    assert K._win_attn_workspace_bytes(lib, "x3", *shape) == K._win_attn_workspace_bytes(lib, "fp32", *shape)
    monkeypatch.setenv("TSPLAT_WINATTN", "32")
    assert lib.tsplat_win_attn_split(*shape) == 0
    assert lib.tsplat_win_attn_workspace_bytes(*shape) == _winattn_bytes(shape, ks_ws)


def test_win_attn_rejects_what_it_rejected(winattn_lib):
    lib = winattn_lib
    for bad in ((0, 64, 64, 1, 2), (1, 64, 64, 0, 2), (1, 64, 64, 1, 0), (1, 63, 64, 1, 2), (1, 64, 66, 1, 2),
                (1, 24, 24, 1, 2)):  # L = 144: no multiple of 64
        assert lib.tsplat_win_attn_split(*bad) == 0
        assert lib.tsplat_win_attn_workspace_bytes(*bad) == 0
        assert lib.tsplat_win_attn_bf16_workspace_bytes(*bad) == 0
    # null pointers are refused before any launch, so these calls need no GPU
    assert lib.tsplat_win_attn_fwd(None, None, None, None, None, 1, 64, 64, 128, 1, 2, 1, None) != 0
    assert lib.tsplat_win_attn_partials_fwd(None, None, None, None, 1, 64, 64, 128, 1, 2, 1, 0, None) != 0
    assert lib.tsplat_win_attn_x3_fwd(None, None, None, None, 1, 64, 64, 128, 1, 2, 1, None) != 0


def test_win_attn_layout_round_trip(tmp_path):
    """winattn_layout.h as host C++: the pixel map and its inverse, and the partials indices tiling the
    workspace (tests/winattn_layout_check.cc), on 16x16, 32x96 (window width 48) and 96x128 maps."""
    import shutil
    import subprocess
    from pathlib import Path
    here = Path(__file__).resolve().parent
    cxx = next((c for c in map(shutil.which, ("c++", "g++", "clang++")) if c), None)
    if cxx is None:  # the HIP compiler the build needs anyway brings a host clang++
        from transplat_amd import build
        cxx = str(Path(build._hipcc()).resolve().parent.parent / "lib" / "llvm" / "bin" / "clang++")
    exe = tmp_path / "winattn_layout_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{here.parent / 'transplat_amd' / 'csrc'}",
                    str(here / "winattn_layout_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout


def test_corr_cell_matches_mmcv(tmp_path):
    """corr_cell.h as host C++ (tests/corr_cell_check.cc): the bilinear cell every sampling kernel goes
    through equals a literal transcription of mmcv's ms_deform_attn_im2col_bilinear -- taken or not, the
    corner, the inside mask, the four weights bit for bit -- on maps 1x1 .. 9x9, 7x5, 12x20 and 64x64 at
    integer positions, their float neighbours, half-integers, +-1e4, +-inf and NaN; a taken sample's
    weights sum to 1 within 2 ulp."""
    import shutil
    import subprocess
    from pathlib import Path
    here = Path(__file__).resolve().parent
    cxx = next((c for c in map(shutil.which, ("c++", "g++", "clang++")) if c), None)
    if cxx is None:  # the HIP compiler the build needs anyway brings a host clang++
        from transplat_amd import build
        cxx = str(Path(build._hipcc()).resolve().parent.parent / "lib" / "llvm" / "bin" / "clang++")
    exe = tmp_path / "corr_cell_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{here.parent / 'transplat_amd' / 'csrc'}",
                    str(here / "corr_cell_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout


def test_wino_layout_walk(tmp_path, winattn_lib):
    """wino_layout.h as host C++ (tests/wino_layout_check.cc): fill_tiles agrees with the launchers' former
    search on 1..40 x 1..140 and the production maps and its regions fit, the packed-U index of each
    precision is injective and in range, the source filler rejects what the launchers rejected; the
    library's buffer sizes are the header's."""
    import shutil
    import subprocess
    from pathlib import Path
    here = Path(__file__).resolve().parent
    cxx = next((c for c in map(shutil.which, ("c++", "g++", "clang++")) if c), None)
    if cxx is None:  # the HIP compiler the build needs anyway brings a host clang++
        from transplat_amd import build
        cxx = str(Path(build._hipcc()).resolve().parent.parent / "lib" / "llvm" / "bin" / "clang++")
    exe = tmp_path / "wino_layout_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{here.parent / 'transplat_amd' / 'csrc'}",
                    str(here / "wino_layout_check.cc"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout
    for co, ci in ((2, 64), (32, 38), (84, 168), (168, 163), (256, 128)):
        cobs, ci_pad = (co + 63) // 64 * 2, (ci + 15) // 16 * 16
        assert winattn_lib.tsplat_wino_weight_floats(co, ci) == 16 * cobs * 32 * ci_pad
        assert winattn_lib.tsplat_wino_weight_bf16x3_bytes(co, ci) == 16 * cobs * 32 * ci_pad * 4
