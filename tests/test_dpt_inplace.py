"""The DPT head's layout copies folded into its split-bf16 1x1s (tsplat_conv1x1_bf16x3_inplace_fwd: token rows
read in place, pixel-shuffled store) and Depth-Anything's depth tail deferred into the depth predictor's fork:
each against the launches it replaces, bit for bit (the operands, products and sum order are the same)."""
from collections import Counter
from contextlib import contextmanager

import pytest
import torch

from transplat_amd import _lib
from transplat_amd import kernels as K
from transplat_amd import synthetic as S


@contextmanager
def entry_points():
    """Counter of the C-ABI entry points called inside the block."""
    names = Counter()
    prev, _lib.ROUTE_HOOK = _lib.ROUTE_HOOK, lambda what, route=None: names.update([what])
    try:
        yield names
    finally:
        _lib.ROUTE_HOOK = prev


def _conv1x1(c, co, device):
    m = torch.nn.Conv2d(c, co, 1).to(device)
    assert K.install_conv2d_dispatch(m) == 1
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("co", [24, 40])
@pytest.mark.parametrize("c", [40, 64])
def test_rows_in_equal_nchw_copy(device, c, co):
    """Tokens [2, 1 + 3 * 5, c] read past the class row (c = 40: a ragged last 16-channel group) against the
    NCHW launch on the permuted copy; the in-place entry point is the one that ran."""
    torch.manual_seed(c + co)
    tokens = torch.randn(2, 1 + 15, c, device=device)
    m = _conv1x1(c, co, device)
    rows = tokens[:, 1:]
    with torch.no_grad(), K.dense_precision("bf16x3"):
        ref = m(rows.permute(0, 2, 1).reshape(2, c, 3, 5).contiguous())
        with entry_points() as r:
            out = K.conv1x1_rows(m, rows, 3, 5)
    assert "tsplat_conv1x1_bf16x3_inplace_fwd" in r and "tsplat_conv2d_bf16x3_fwd" not in r, r
    assert out.shape == ref.shape == (2, co, 3, 5)
    assert torch.equal(out, ref)


@pytest.mark.gpu
def test_rows_in_fallbacks_equal(device):
    """A base that is not 16-byte aligned, a channel count that is no multiple of 8, the switch off and a module
    without the installed forward all take the copy and the plain launch: still equal, and no in-place launch."""
    torch.manual_seed(3)
    buf = torch.randn(2 * 16 * 40 + 1, device=device)
    cases = {"misaligned": (buf[1:].view(2, 16, 40)[:, 1:], 40), "c = 36": (torch.randn(2, 16, 36, device=device)[:, 1:], 36),
             "switched off": (torch.randn(2, 16, 40, device=device)[:, 1:], 40)}
    assert cases["misaligned"][0].data_ptr() % 16 == 4
    for name, (rows, c) in cases.items():
        m = _conv1x1(c, 24, device)
        was = K._ROWS_IN
        K._ROWS_IN = name != "switched off"
        try:
            with torch.no_grad(), K.dense_precision("bf16x3"), entry_points() as r:
                out = K.conv1x1_rows(m, rows, 3, 5)
                ref = m(rows.permute(0, 2, 1).reshape(2, c, 3, 5).contiguous())
        finally:
            K._ROWS_IN = was
        assert "tsplat_conv1x1_bf16x3_inplace_fwd" not in r, name
        assert torch.equal(out, ref), name
    plain = torch.nn.Conv2d(40, 24, 1).to(device)  # the module's own forward: nothing of ours replaces it
    rows = cases["switched off"][0]
    with torch.no_grad(), K.dense_precision("bf16x3"):
        assert torch.equal(K.conv1x1_rows(plain, rows, 3, 5), plain(rows.permute(0, 2, 1).reshape(2, 40, 3, 5).contiguous()))


@pytest.mark.gpu
@pytest.mark.parametrize("oc", [6, 24])
@pytest.mark.parametrize("k", [2, 4])
def test_shuffle_out_equals_copy(device, k, oc):
    """ConvTranspose2d(kernel = stride = k) on a 3 x 5 map of two images: the 1x1 with the pixel-shuffled store
    against the 1x1 + F.pixel_shuffle's copy (the switch off), and against float64 at the direct kernel's bar."""
    torch.manual_seed(10 * k + oc)
    ci = 16
    x = torch.randn(2, ci, 3, 5, device=device)
    wt = torch.randn(ci, oc, k, k, device=device) / ci ** 0.5
    b = torch.randn(oc, device=device)
    with torch.no_grad(), K.dense_precision("bf16x3"):
        out = K.conv_transpose_direct(x, wt, b, k)
        was, K._SHUFFLE_OUT = K._SHUFFLE_OUT, False
        try:
            ref = K.conv_transpose_direct(x, wt, b, k)
        finally:
            K._SHUFFLE_OUT = was
    assert out.shape == ref.shape == (2, oc, 3 * k, 5 * k)
    assert torch.equal(out, ref)
    r64 = torch.nn.functional.conv_transpose2d(x.double(), wt.double(), b.double(), stride=k)
    assert (out.double() - r64).abs().max().item() <= 2e-5 * r64.abs().max().item()


@pytest.mark.gpu
def test_inplace_entry_rejects_bad_arguments(device):
    """One layout per launch; channel-last rows need whole, aligned 8-channel runs; shuffle 2 or 4 dividing c_out."""
    lib = _lib.load()
    p = torch.zeros(4096, device=device).data_ptr()
    call = lambda ci, px, img, co, shuf, x=p: lib.tsplat_conv1x1_bf16x3_inplace_fwd(  # noqa: E731
        x, ci, px, img, p, None, p, 1, 4, 4, co, shuf, 1, 1, None, None, None)
    assert call(16, 0, 0, 32, 0) == -1 and call(16, 16, 256, 32, 2) == -1  # neither / both
    assert call(12, 12, 192, 32, 0) == -1 and call(16, 18, 288, 32, 0) == -1 and call(16, 16, 254, 32, 0) == -1
    assert call(16, 16, 128, 32, 0) == -1  # images overlap
    assert call(16, 16, 256, 32, 0, p + 4) == -1  # misaligned base
    assert call(16, 0, 0, 32, 3) == -1 and call(16, 0, 0, 24, 4) == -1 and call(16, 0, 64, 32, 2) == -1


def _head(device):
    """A DPT head with random weights on a 4 x 4 patch grid (branch 3: 4^2 -> 2^2), conv dispatch installed."""
    from transplat_amd.model.depth_anything.dpt import DPTHead

    torch.manual_seed(0)
    head = DPTHead(64, features=32, out_channels=(16, 32, 64, 64)).to(device).eval()
    K.install_conv2d_dispatch(head)
    tokens = [torch.randn(2, 1 + 16, 64, device=device) for _ in range(4)]
    return head, [(t[:, 1:], t[:, 0]) for t in tokens]


@pytest.mark.gpu
def test_dpt_head_inplace_equals_copies(device):
    """The whole head with both switches on against both off: depth and out_feature bit for bit; on, no token or
    shuffle copy is left in reassemble (the four projects and the two transposed convolutions run in place)."""
    head, feats = _head(device)
    was = K._ROWS_IN, K._SHUFFLE_OUT
    try:
        with torch.no_grad(), K.dense_precision("bf16x3"):
            with entry_points() as r:
                d1, f1 = head(feats, 4, 4)
            K._ROWS_IN = K._SHUFFLE_OUT = False
            d0, f0 = head(feats, 4, 4)
    finally:
        K._ROWS_IN, K._SHUFFLE_OUT = was
    assert r["tsplat_conv1x1_bf16x3_inplace_fwd"] == 6, r
    assert torch.equal(d1, d0) and torch.equal(f1, f0)
    assert torch.isfinite(d1).all() and d1.abs().max().item() > 0


@pytest.mark.gpu
def test_dpt_head_deferred_tail_equals_forward(device):
    head, feats = _head(device)
    with torch.no_grad(), K.dense_precision("bf16x3"):
        d0, f0 = head(feats, 4, 4, raw_tail=True)
        final_out, f1 = head(feats, 4, 4, raw_tail=True, defer_tail=True)
        d1 = head.depth_tail(final_out, 4, 4, raw_tail=True)
    assert torch.equal(d1, d0) and torch.equal(f1, f0)


@pytest.fixture(scope="module")
def encoder_case(device):
    """The e2e test's configuration (bf16x3, one scene, 256 x 256) and the eager encoder step with the depth tail
    where it was (switch off): computed once, left unchanged."""
    from transplat_amd.e2e import build_model
    from transplat_amd.gemm_tuning import use_tuned_gemms
    from transplat_amd.model.encoder import encoder_trans as E

    use_tuned_gemms(device, "bf16x3")
    model = build_model(device, "bf16x3")
    ctx = model.data_shim(S.make_batch(1, image_shape=(256, 256), device=device))["context"]
    was, E._DEFER_DA_TAIL = E._DEFER_DA_TAIL, False
    try:
        with torch.no_grad():
            g = model.encoder(ctx, 0, deterministic=True)
            off = [t.float().clone() for t in (g.means, g.covariances, g.harmonics, g.opacities)]
    finally:
        E._DEFER_DA_TAIL = was
    torch.cuda.synchronize()
    return model, ctx, off


@pytest.mark.gpu
def test_encoder_deferred_tail_equals_serial_tail(encoder_case):
    """The depth tail inside the projection's fork: the four Gaussian tensors of an eager step, bit for bit."""
    from transplat_amd.model.encoder import encoder_trans as E

    model, ctx, off = encoder_case
    assert E._DEFER_DA_TAIL
    with torch.no_grad():
        g = model.encoder(ctx, 0, deterministic=True)
    for name, a, b in zip(("means", "covariances", "harmonics", "opacities"),
                          (g.means, g.covariances, g.harmonics, g.opacities), off):
        assert torch.equal(a.float(), b), name


@pytest.mark.gpu
def test_encoder_deferred_tail_graph_replays_equal_eager(encoder_case):
    """Three hipGraph replays of the encoder step with the tail in the fork equal the eager step."""
    model, ctx, off = encoder_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            model.encoder(ctx, 0, deterministic=True)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g = model.encoder(ctx, 0, deterministic=True)
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("means", "covariances", "harmonics", "opacities"),
                              (g.means, g.covariances, g.harmonics, g.opacities), off):
            assert torch.equal(a.float(), b), (i, name)
