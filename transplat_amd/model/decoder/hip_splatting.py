"""Camera setup + call of the gfx950 Gaussian rasterizer (replaces reference `render_cuda`).

Reference: src/model/decoder/cuda_splatting.py:26-136. The reference repeats the Gaussians
over every target view, then loops the views in Python (two `.item()` host syncs per view) and
calls the third-party CUDA rasterizer once per view. Here the per-view camera constants are
computed once on the device (same torch expressions as the reference) and every view of every
scene is rasterized by one `tsplat_raster_fwd` call that reads the un-repeated Gaussian buffers.
"""
from __future__ import annotations

from dataclasses import dataclass
from math import isqrt

import torch
from torch import Tensor

from ... import kernels
from ... import _lib
from ...geometry.projection import get_fov


def get_projection_matrix(near: Tensor, far: Tensor, fov_x: Tensor, fov_y: Tensor) -> Tensor:
    """(reference cuda_splatting.py:26-53) x/y -> (-1, 1), z -> (0, 1)."""
    tan_fov_x = (0.5 * fov_x).tan()
    tan_fov_y = (0.5 * fov_y).tan()
    top = tan_fov_y * near
    bottom = -top
    right = tan_fov_x * near
    left = -right
    (b,) = near.shape
    result = torch.zeros((b, 4, 4), dtype=torch.float32, device=near.device)
    result[:, 0, 0] = 2 * near / (right - left)
    result[:, 1, 1] = 2 * near / (top - bottom)
    result[:, 0, 2] = (right + left) / (right - left)
    result[:, 1, 2] = (top + bottom) / (top - bottom)
    result[:, 3, 2] = 1
    result[:, 2, 2] = far / (far - near)
    result[:, 2, 3] = -(far * near) / (far - near)
    return result


@dataclass
class RasterCameras:
    """Per-view constants in the layouts of `tsplat_raster_fwd` (all fp32, contiguous)."""

    viewmat: Tensor  # [V, 16] column-major view matrix (= inverse(c2w)^T row-major)
    projmat: Tensor  # [V, 16] column-major full projection
    campos: Tensor  # [V, 3]
    tanfov: Tensor  # [V, 2]
    bg: Tensor  # [V, 3]
    scale: Tensor  # [V, 2] (s, s^2), s = 1/near when scale-invariant, else 1

    def to(self, device) -> "RasterCameras":
        return RasterCameras(*(getattr(self, f).to(device) for f in self.__dataclass_fields__))


def prepare_cameras(
    extrinsics: Tensor,
    intrinsics: Tensor,
    near: Tensor,
    far: Tensor,
    background_color: Tensor,
    scale_invariant: bool = True,
) -> RasterCameras:
    """Camera math of render_cuda (cuda_splatting.py:73-96) for V = (b v) flattened views. Device
    tensors: one launch (tsplat_raster_cameras); host tensors (the oracle / CPU-baseline callers)
    take the same math on torch ops."""
    if extrinsics.is_cuda:
        lib = _lib.load()
        v = extrinsics.shape[0]
        dev = extrinsics.device
        f = lambda t: t.float().contiguous()
        ext, intr, nr, fr, bg = f(extrinsics), f(intrinsics), f(near), f(far), f(background_color)
        out = [torch.empty((v, n), dtype=torch.float32, device=dev) for n in (16, 16, 3, 2, 3, 2)]
        rc = lib.tsplat_raster_cameras(_lib.ptr(ext), _lib.ptr(intr), _lib.ptr(nr), _lib.ptr(fr), _lib.ptr(bg),
                                       int(bg.dim() == 2), int(scale_invariant), v, *(_lib.ptr(t) for t in out),
                                       _lib.stream_ptr(dev))
        _lib.check(rc, "tsplat_raster_cameras")
        return RasterCameras(*out)
    extrinsics = extrinsics.float()
    if scale_invariant:
        scale = 1 / near
        extrinsics = extrinsics.clone()
        extrinsics[..., :3, 3] = extrinsics[..., :3, 3] * scale[:, None]
        near = near * scale
        far = far * scale
    else:
        scale = torch.ones_like(near)
    fov_x, fov_y = get_fov(intrinsics).unbind(dim=-1)
    tan_fov_x = (0.5 * fov_x).tan()
    tan_fov_y = (0.5 * fov_y).tan()
    projection_matrix = get_projection_matrix(near, far, fov_x, fov_y).transpose(1, 2)
    view_matrix = kernels.small_inverse(extrinsics).transpose(1, 2)
    full_projection = view_matrix @ projection_matrix
    v = extrinsics.shape[0]
    return RasterCameras(
        viewmat=view_matrix.contiguous().view(v, 16),
        projmat=full_projection.contiguous().view(v, 16),
        campos=extrinsics[:, :3, 3].contiguous(),
        tanfov=torch.stack((tan_fov_x, tan_fov_y), dim=-1).contiguous(),
        bg=background_color.float().contiguous(),
        scale=torch.stack((scale, scale * scale), dim=-1).float().contiguous(),
    )


class _RasterState:
    """Per-device workspace + sticky overflow status, grown on demand. A superseded workspace is
    retired, not freed: a captured hipGraph may still hold its address."""

    def __init__(self):
        self.workspace: dict = {}
        self.status: dict = {}
        self.last: dict = {}
        self.retired: list = []

    def get(self, device, nbytes: int):
        key = (device.type, device.index)
        ws = self.workspace.get(key)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                self.retired.append(ws)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self.workspace[key] = ws
        st = self.status.get(key)
        if st is None:
            st = torch.zeros(1, dtype=torch.int32, device=device)
            self.status[key] = st
        return ws, st


_STATE = _RasterState()


MAX_CAPACITY = 1 << 30  # 8 GiB of 8-byte instance keys


def default_capacity(num_gaussians: int, num_views: int, height: int, width: int) -> int:
    """The worst case, every Gaussian touching every 16x16 tile of every view, so a captured
    graph can never overflow (the reference sizes its buffers from a host readback of the exact
    count instead, which a graph cannot do). 8 bytes per instance: 0.8 GB for one 256x256 scene
    x 3 views, 6.4 GB at batch 8, a small slice of 288 GB. Larger problems are capped at
    MAX_CAPACITY and rely on the overflow status."""
    tiles = ((height + 15) // 16) * ((width + 15) // 16)
    return max(1, min(num_gaussians * num_views * tiles, MAX_CAPACITY))


DEPTH_MODES = {"depth": 0, "disparity": 1, "relative_disparity": 2, "log": 3}  # tsplat_raster_depth_fwd


@dataclass
class RasterOutput:
    """What `rasterize_with_depth` returns; an output that was not asked for is None."""

    color: Tensor | None  # [V, 3, H, W]
    radii: Tensor  # [V, G] int32
    depth: Tensor | None  # [V, H, W]
    alpha: Tensor | None  # [V, H, W]


def _rasterize(means, covariances, harmonics, opacities, cameras, image_shape, views_per_scene, sh_degree,
               capacity, check, debug, extra=None, keep=None) -> RasterOutput:
    """The call behind rasterize() (extra None: tsplat_raster_fwd) and rasterize_with_depth()
    (extra = (near, far, mode id, color, depth, alpha): tsplat_raster_depth_fwd), with the same
    capacity, overflow and debug rules. keep: a list that receives what a backward needs (the
    descriptor, the fp32 contiguous inputs and camera arrays the call read, its workspace, its near and
    far planes); the call then runs on a workspace tensor of its own instead of the device's shared
    one, which the next call overwrites."""
    lib = _lib.load()
    s, g, _ = means.shape
    m = harmonics.shape[-1]
    v = cameras.viewmat.shape[0]
    if v != s * views_per_scene:
        raise ValueError(f"{v} views for {s} scenes x {views_per_scene} views per scene")
    if covariances.shape != (s, g, 3, 3) or harmonics.shape[:3] != (s, g, 3) or opacities.shape != (s, g):
        raise ValueError("Gaussian tensor shapes disagree")
    if sh_degree is None:
        sh_degree = min(isqrt(m) - 1, 3)
    h, w = image_shape
    dev = means.device
    f32 = lambda t: t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()
    means, covariances, harmonics, opacities = map(f32, (means, covariances, harmonics, opacities))
    if capacity is None:
        capacity = default_capacity(g, v, h, w)
    nbytes = int(lib.tsplat_raster_workspace_bytes(g, v, h, w, capacity))
    if keep is not None:
        _lib.ptr(means)  # raises for host tensors before anything is allocated
        ws, status = torch.empty(nbytes, dtype=torch.uint8, device=dev), _STATE.get(dev, 0)[1]
    else:
        ws, status = _STATE.get(dev, nbytes)
    want_color, want_depth, want_alpha = (True, False, False) if extra is None else extra[3:]
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    color = new(v, 3, h, w) if want_color else None
    depth = new(v, h, w) if want_depth else None
    alpha = new(v, h, w) if want_alpha else None
    radii = torch.empty((v, g), dtype=torch.int32, device=dev)
    desc = _lib.RasterDesc(g, v, views_per_scene, h, w, m, sh_degree, capacity)
    cams = [f32(cameras.viewmat), f32(cameras.projmat), f32(cameras.campos), f32(cameras.tanfov),
            f32(cameras.bg), f32(cameras.scale)]
    planes = []
    if extra is not None:
        planes = [None if t is None else f32(t).reshape(-1) for t in extra[:2]]
        for t in planes:
            if t is not None and t.shape != (v,):
                raise ValueError(f"near / far must hold one value per view ({v})")
    for t in cams + [t for t in planes if t is not None]:
        if t.device != dev:
            raise ValueError("camera tensors must be on the Gaussians' device")
    name = "tsplat_raster_fwd" if extra is None else "tsplat_raster_depth_fwd"
    if debug and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("rasterize(debug=True) synchronises after every launch: not inside hipGraph capture")
    was = lib.tsplat_set_debug(1) if debug else None
    try:
        gauss = [_lib.ptr(t) for t in (means, covariances, harmonics, opacities)]
        tail = (_lib.ptr(radii), _lib.ptr(ws), _lib.ptr(status), _lib.stream_ptr(dev))
        if extra is None:
            rc = lib.tsplat_raster_fwd(desc, *gauss, *(_lib.ptr(t) for t in cams), _lib.ptr(color), *tail)
        else:
            rc = lib.tsplat_raster_depth_fwd(desc, *gauss, *(_lib.ptr(t) for t in cams),
                                             *(_lib.ptr(t) for t in planes), extra[2],
                                             _lib.ptr(color), _lib.ptr(depth), _lib.ptr(alpha), *tail)
    finally:
        if was is not None:
            lib.tsplat_set_debug(was)
    _lib.check(rc, name)
    _STATE.last[(dev.type, dev.index)] = (ws, int(lib.tsplat_raster_num_rendered_offset(g, v, h, w)))
    if check:
        check_status(dev)
    if keep is not None:
        keep[:] = [desc, (means, covariances, harmonics, opacities), cams, ws, planes]
    return RasterOutput(color, radii, depth, alpha)


def rasterize(
    means: Tensor,
    covariances: Tensor,
    harmonics: Tensor,
    opacities: Tensor,
    cameras: RasterCameras,
    image_shape: tuple[int, int],
    views_per_scene: int,
    sh_degree: int | None = None,
    capacity: int | None = None,
    check: bool = True,
    debug: bool = False,
) -> tuple[Tensor, Tensor]:
    """Render V = scenes * views_per_scene views.

    debug=True mirrors the upstream rasterizer's `debug` setting (cuda_splatting.py:120): every
    launch of the call is followed by a device synchronisation and an error check
    (tsplat_set_debug), so a faulting kernel is named; it cannot run inside hipGraph capture.

    means [S, G, 3], covariances [S, G, 3, 3], harmonics [S, G, 3, M], opacities [S, G]
    -> color [V, 3, H, W], radii [V, G] int32.
    `sh_degree` defaults to isqrt(M) - 1 (the degree render_cuda passes) capped at the
    evaluated degree of the upstream rasterizer (3); pass 4 to evaluate degree-4 terms.
    """
    out = _rasterize(means, covariances, harmonics, opacities, cameras, image_shape, views_per_scene, sh_degree,
                     capacity, check, debug)
    return out.color, out.radii


def _depth_extra(caller: str, near, far, depth_mode, color, alpha) -> tuple:
    """The checked `extra` of _rasterize() for rasterize_with_depth() and its differentiable form:
    (near, far, mode id, color, depth, alpha)."""
    if depth_mode is not None and depth_mode not in DEPTH_MODES:
        raise ValueError(f"depth_mode {depth_mode!r}: expected one of {sorted(DEPTH_MODES)} or None")
    want_depth = depth_mode is not None
    if not (color or want_depth or alpha):
        raise ValueError(f"{caller}: no output asked for")
    if want_depth and (near is None or far is None):
        raise ValueError("a depth render needs the views' near and far planes")
    return near, far, DEPTH_MODES[depth_mode] if want_depth else 0, bool(color), want_depth, bool(alpha)


def rasterize_with_depth(
    means: Tensor,
    covariances: Tensor,
    harmonics: Tensor,
    opacities: Tensor,
    cameras: RasterCameras,
    image_shape: tuple[int, int],
    views_per_scene: int,
    sh_degree: int | None = None,
    capacity: int | None = None,
    check: bool = True,
    debug: bool = False,
    *,
    near: Tensor | None = None,
    far: Tensor | None = None,
    depth_mode: str | None = "depth",
    color: bool = True,
    alpha: bool = False,
) -> RasterOutput:
    """rasterize() with rendered depth and accumulated opacity from the same pass
    (tsplat_raster_depth_fwd; replaces the second rasterizer run of the reference's
    render_depth_cuda, cuda_splatting.py:375-417).

    near / far [V]: the views' unscaled planes (what prepare_cameras took). `depth_mode`: one of
    DEPTH_MODES -> depth [V, H, W], the reference's depth render (the blend of max(C0 f + 0.5, 0)
    over black, f the mode's function of the camera-space depth); None: no depth. alpha=True ->
    alpha [V, H, W] = 1 - T, the accumulated opacity. color=False skips the colours (the SH
    coefficients are not read). Colour and radii are bit-identical to rasterize()'s.
    """
    extra = _depth_extra("rasterize_with_depth", near, far, depth_mode, color, alpha)
    return _rasterize(means, covariances, harmonics, opacities, cameras, image_shape, views_per_scene, sh_degree,
                      capacity, check, debug, extra)


class _RasterizeFn(torch.autograd.Function):
    """_rasterize() with a backward, for both differentiable calls: the forward entry point on a private
    workspace, then the matching backward on what that call left in it (extra None: tsplat_raster_fwd /
    tsplat_raster_bwd, else tsplat_raster_depth_fwd / tsplat_raster_depth_bwd). Returns (color, depth,
    alpha, radii); an output that was not asked for is None; an output the loss does not use arrives in
    backward() as None and goes to the library as NULL."""

    @staticmethod
    def forward(ctx, means, covariances, harmonics, opacities, cameras, image_shape, views_per_scene, sh_degree,
                capacity, check, debug, extra):
        keep = []
        out = _rasterize(means, covariances, harmonics, opacities, cameras, image_shape, views_per_scene, sh_degree,
                         capacity, check, debug, extra, keep=keep)
        desc, gauss, cams, ws, planes = keep
        ctx.desc, ctx.workspace, ctx.mode = desc, ws, None if extra is None else extra[2]
        ctx.dtypes = tuple(t.dtype for t in (means, covariances, harmonics, opacities))
        ctx.save_for_backward(*gauss, *cams, *(planes or (None, None)), out.color, out.depth, out.alpha, out.radii)
        ctx.mark_non_differentiable(out.radii)
        ctx.set_materialize_grads(False)
        return out.color, out.depth, out.alpha, out.radii

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_color, grad_depth, grad_alpha, _grad_radii):
        lib = _lib.load()
        t = ctx.saved_tensors
        gauss, cams, planes, outs, radii = t[:4], t[4:10], t[10:12], t[12:15], t[15]
        dev = radii.device
        desc = ctx.desc
        none = (None,) * 12
        gin = [None if g is None or o is None else g.float().contiguous()
               for g, o in zip((grad_color, grad_depth, grad_alpha), outs)]
        grads = [torch.empty_like(x) if need else None for x, need in zip(gauss, ctx.needs_input_grad[:4])]
        if all(g is None for g in grads) or all(g is None for g in gin):
            return none
        outs = [o if g is not None else None for o, g in zip(outs, gin)]
        bws = torch.empty(int(lib.tsplat_raster_bwd_workspace_bytes(desc.num_gaussians, desc.num_views)),
                          dtype=torch.uint8, device=dev)
        p = _lib.ptr
        head = (desc, *(p(x) for x in gauss), *(p(x) for x in cams))
        tail = (p(radii), p(ctx.workspace), p(bws), *(p(g) for g in grads), _lib.stream_ptr(dev))
        if ctx.mode is None:
            name, rc = "tsplat_raster_bwd", lib.tsplat_raster_bwd(*head, p(outs[0]), p(gin[0]), *tail)
        else:
            name, rc = "tsplat_raster_depth_bwd", lib.tsplat_raster_depth_bwd(
                *head, *(p(x) for x in planes), ctx.mode, *(p(x) for x in outs), *(p(x) for x in gin), *tail)
        _lib.check(rc, name)
        grads = [None if g is None else g.to(dt) for g, dt in zip(grads, ctx.dtypes)]
        return (*grads, *none[4:])


def rasterize_differentiable(
    means: Tensor,
    covariances: Tensor,
    harmonics: Tensor,
    opacities: Tensor,
    cameras: RasterCameras,
    image_shape: tuple[int, int],
    views_per_scene: int,
    sh_degree: int | None = None,
    capacity: int | None = None,
    check: bool = True,
    debug: bool = False,
) -> tuple[Tensor, Tensor]:
    """rasterize() whose colour is differentiable in the four Gaussian tensors (the reference's
    rasterizer has a backward; render_cuda hands it means3D, cov3D_precomp, shs and opacities).

    Same arguments and the same (color, radii), bit for bit. The forward runs on a workspace tensor
    of its own, kept with the inputs, the camera arrays, color and radii for the backward
    (tsplat_raster_bwd): the exact vector-Jacobian product with every discrete decision of the
    forward held fixed, for the inputs that require grad. radii is not differentiable; there is no
    double backward; cameras and background get no gradient. The per-pixel sums are float atomic
    adds, so the last bits of a gradient can differ between two runs.
    """
    color, _, _, radii = _RasterizeFn.apply(means, covariances, harmonics, opacities, cameras, image_shape,
                                            views_per_scene, sh_degree, capacity, check, debug, None)
    return color, radii


def rasterize_with_depth_differentiable(
    means: Tensor,
    covariances: Tensor,
    harmonics: Tensor,
    opacities: Tensor,
    cameras: RasterCameras,
    image_shape: tuple[int, int],
    views_per_scene: int,
    sh_degree: int | None = None,
    capacity: int | None = None,
    check: bool = True,
    debug: bool = False,
    *,
    near: Tensor | None = None,
    far: Tensor | None = None,
    depth_mode: str | None = "depth",
    color: bool = True,
    alpha: bool = False,
) -> RasterOutput:
    """rasterize_with_depth() whose colour, depth and alpha are differentiable in the four Gaussian
    tensors (the reference trains through render_depth_cuda's depth as through the colour).

    Same arguments and the same RasterOutput, bit for bit. The forward runs on a workspace tensor of
    its own, kept with the inputs, the camera arrays, near and far, the outputs and radii for the
    backward (tsplat_raster_depth_bwd): one fused pass over colour, depth and alpha gradients, the
    exact vector-Jacobian product with every discrete decision of the forward held fixed. The depth
    value's own derivative reaches the means; covariances, opacities and harmonics get depth and alpha
    gradient through the blend weights only. An output the loss does not use costs nothing. radii is
    not differentiable; there is no double backward; cameras, background, near and far get no
    gradient. The per-pixel sums are float atomic adds, so the last bits of a gradient can differ
    between two runs.
    """
    extra = _depth_extra("rasterize_with_depth_differentiable", near, far, depth_mode, color, alpha)
    c, d, a, radii = _RasterizeFn.apply(means, covariances, harmonics, opacities, cameras, image_shape,
                                        views_per_scene, sh_degree, capacity, check, debug, extra)
    return RasterOutput(c, radii, d, a)


MAX_VIEWS_PER_CALL = 32  # the rasterizer's per-scene view mask is 32 bits wide


def plan_view_groups(b: int, v: int, views_per_call: int) -> list[slice]:
    """The view slices of the rasterizer calls that render v views of each of b scenes: one call for
    v <= 32 (the rasterizer's limit per scene), else groups of views_per_call (1..32) views in order,
    the last one shorter. Each call renders its slice of every scene."""
    if b < 1 or v < 1:
        raise ValueError(f"plan_view_groups: {b} scenes x {v} views")
    if v <= MAX_VIEWS_PER_CALL:
        return [slice(0, v)]
    if not 1 <= views_per_call <= MAX_VIEWS_PER_CALL:
        raise ValueError(f"views_per_call {views_per_call}: expected 1..{MAX_VIEWS_PER_CALL}")
    return [slice(s, min(s + views_per_call, v)) for s in range(0, v, views_per_call)]


def select_view_rows(rows: Tensor, b: int, v: int, views: slice) -> Tensor:
    """The rows of a group from (b v)-ordered per-view rows [b * v, ...]: views `views` of every scene,
    (b g)-ordered. A view of the input for b = 1, one gather copy otherwise; no host sync."""
    if views == slice(0, v):
        return rows
    return rows.reshape(b, v, *rows.shape[1:])[:, views].reshape(-1, *rows.shape[1:])


def merge_view_groups(parts: list[Tensor], b: int) -> Tensor:
    """Inverse of select_view_rows over a whole plan: per-group outputs [(b g), ...] in plan order ->
    [(b v), ...]."""
    if len(parts) == 1:
        return parts[0]
    if b == 1:
        return torch.cat(parts, dim=0)
    merged = torch.cat([p.reshape(b, -1, *p.shape[1:]) for p in parts], dim=1)
    return merged.reshape(-1, *merged.shape[2:])


def num_rendered(device) -> int:
    """(Gaussian, tile) instances generated by the last rasterize() on `device` (the reference
    forward's num_rendered; syncs)."""
    ws, off = _STATE.last[(device.type, device.index)]
    return int(ws[off:off + 4].view(torch.int32).item())


def status_tensor(device):
    """The device's sticky overflow flag (int32 [1]; None before the first rasterize) -- read
    without a sync by copying it on the stream."""
    return _STATE.status.get((device.type, device.index))


def check_status(device) -> None:
    """Raise if any rasterizer call on `device` overflowed its instance capacity (syncs)."""
    st = _STATE.status.get((device.type, device.index))
    if st is not None and int(st.item()) != 0:
        st.zero_()
        raise RuntimeError("tsplat_raster_fwd: instance capacity exceeded; pass a larger capacity")
