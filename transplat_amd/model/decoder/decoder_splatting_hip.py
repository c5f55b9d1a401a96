"""`splatting_hip` decoder: drop-in for DecoderSplattingCUDA
(reference src/model/decoder/decoder_splatting_cuda.py:26-97).

Differences by design: the Gaussians are NOT repeated per target view (the reference
materialises V copies, 46 MB each at G = 131072); all (b v) views go to one rasterizer call, and
the depth render of `depth_mode` comes out of that same call (the reference runs the rasterizer a
second time over fake colours). More than 32 views per scene (a video trajectory) are rendered in
groups of `views_per_call` views per scene, one rasterizer call each on the one shared workspace.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Literal, Optional

import torch
from einops import rearrange, repeat
from torch import Tensor

from ..types import Gaussians
from .decoder import Decoder, DecoderOutput, DepthRenderingMode
from .hip_splatting import (RasterCameras, RasterOutput, check_status, merge_view_groups, plan_view_groups,
                            prepare_cameras, rasterize, rasterize_differentiable, rasterize_with_depth,
                            rasterize_with_depth_differentiable, select_view_rows)


@dataclass
class DecoderSplattingHIPCfg:
    name: Literal["splatting_hip", "splatting_cuda"] = "splatting_hip"
    sh_eval_degree: Optional[int] = None  # None: min(isqrt(d_sh) - 1, 3), the upstream behaviour
    check_overflow: bool = True  # sync after each call to surface capacity overflow
    debug: bool = False  # upstream GaussianRasterizationSettings.debug: sync + check after every launch
    # views per scene of one rasterizer call when a scene has more than 32 (1..32): at the production
    # scene 16 keeps the worst-case instance keys at 4 GiB, half the MAX_CAPACITY cap
    views_per_call: int = 16
    # True: while grad is enabled and a Gaussian tensor requires grad, the colour comes from
    # rasterize_differentiable (tsplat_raster_bwd as its backward) and carries a grad_fn. Without
    # differentiable_depth there are no depth gradients: depth_mode then raises NotImplementedError.
    # False: the forward-only calls.
    differentiable: bool = False
    # True (needs differentiable=True): under the same conditions forward(depth_mode=m) returns colour
    # and depth from one rasterize_with_depth_differentiable call per view group (tsplat_raster_depth_bwd
    # as its backward), both with a grad_fn, and render_depth() the depth-only call's.
    differentiable_depth: bool = False

    def __post_init__(self):
        if self.differentiable_depth and not self.differentiable:
            raise ValueError("DecoderSplattingHIPCfg: differentiable_depth=True needs differentiable=True")


def _depth_fused() -> bool:
    """A/B knob, read per call: TSPLAT_DEPTH_FUSED=0 renders depth by the two-pass route."""
    return os.environ.get("TSPLAT_DEPTH_FUSED", "1") != "0"


def depth_fake_color(extrinsics: Tensor, means: Tensor, near: Tensor, far: Tensor,
                     mode: DepthRenderingMode = "depth") -> Tensor:
    """Per-view fake colour of the depth render (reference cuda_splatting.py:388-401):
    extrinsics [V, 4, 4] c2w, means [V, G, 3], near / far [V] -> [V, G]. The "log" mode keeps the
    reference's minimum(near).maximum(far) order."""
    cam = torch.einsum("bij,bgj->bgi", extrinsics.inverse(), torch.cat([means, torch.ones_like(means[..., :1])], -1))
    fake = cam[..., 2]
    if mode == "disparity":
        fake = 1 / fake
    elif mode == "relative_disparity":
        eps = 1e-10  # depth_to_relative_disparity (reference matching/conversions.py:18-28)
        disp_near, disp_far = 1 / (near[:, None] + eps), 1 / (far[:, None] + eps)
        fake = 1 - (1 / (fake + eps) - disp_far) / (disp_near - disp_far + eps)
    elif mode == "log":
        fake = fake.minimum(near[:, None]).maximum(far[:, None]).log()
    return fake


class DecoderSplattingHIP(Decoder[DecoderSplattingHIPCfg]):
    background_color: Tensor

    def __init__(self, cfg: DecoderSplattingHIPCfg, dataset_cfg) -> None:
        super().__init__(cfg, dataset_cfg)
        self.register_buffer(
            "background_color",
            torch.tensor(dataset_cfg.background_color, dtype=torch.float32),
            persistent=False,
        )

    def forward(
        self,
        gaussians: Gaussians,
        extrinsics: Tensor,
        intrinsics: Tensor,
        near: Tensor,
        far: Tensor,
        image_shape: tuple[int, int],
        depth_mode: DepthRenderingMode | None = None,
    ) -> DecoderOutput:
        b, v, _, _ = extrinsics.shape
        if self._wants_grad(gaussians):
            if depth_mode is not None and not self.cfg.differentiable_depth:
                raise NotImplementedError(
                    "DecoderSplattingHIP(differentiable=True): gradients of the depth render need "
                    "differentiable_depth=True; call with depth_mode=None, or under torch.no_grad() for a depth "
                    "without gradients")
            rgb, depth = self._render_differentiable(gaussians, extrinsics, intrinsics, near, far, image_shape,
                                                     depth_mode)
            return DecoderOutput(rearrange(rgb, "(b v) c h w -> b v c h w", b=b, v=v),
                                 None if depth is None else rearrange(depth, "(b v) h w -> b v h w", b=b, v=v))
        fused = depth_mode is not None and _depth_fused()
        out = self._render(gaussians, extrinsics, intrinsics, near, far, image_shape,
                           depth_mode if fused else None, color=True)
        color = rearrange(out.color, "(b v) c h w -> b v c h w", b=b, v=v)
        depth = None
        if fused:
            depth = rearrange(out.depth, "(b v) h w -> b v h w", b=b, v=v)
        elif depth_mode is not None:
            depth = self.render_depth(gaussians, extrinsics, intrinsics, near, far, image_shape, depth_mode)
        return DecoderOutput(color, depth)

    def _wants_grad(self, gaussians: Gaussians) -> bool:
        """cfg.differentiable, grad enabled, and a Gaussian tensor that requires grad."""
        return (self.cfg.differentiable and torch.is_grad_enabled() and any(
            t.requires_grad for t in (gaussians.means, gaussians.covariances, gaussians.harmonics,
                                      gaussians.opacities)))

    def _render_differentiable(self, gaussians, extrinsics, intrinsics, near, far, image_shape, depth_mode=None,
                               color=True):
        """The outputs of _render() with a grad_fn -> (colour [(b v), 3, H, W] or None, depth [(b v), H, W] or
        None): rasterize_differentiable without a depth mode, else one rasterize_with_depth_differentiable call
        for colour and depth together (color=False: the depth-only call). More than 32 views per scene go group
        by group, each call on a workspace of its own; autograd sums the groups' gradients."""
        b, v, _, _ = extrinsics.shape
        nr = rearrange(near, "b v -> (b v)")
        fr = rearrange(far, "b v -> (b v)")
        cams = prepare_cameras(
            rearrange(extrinsics, "b v i j -> (b v) i j"),
            rearrange(intrinsics, "b v i j -> (b v) i j"),
            nr,
            fr,
            repeat(self.background_color, "c -> (b v) c", b=b, v=v),
        )
        gauss = (gaussians.means, gaussians.covariances, gaussians.harmonics, gaussians.opacities)
        groups = plan_view_groups(b, v, self.cfg.views_per_call)
        single = len(groups) == 1
        colors, depths = [], []
        for views in groups:
            pick = lambda t: select_view_rows(t, b, v, views)
            c = cams if single else RasterCameras(*(pick(getattr(cams, f)) for f in cams.__dataclass_fields__))
            kw = dict(views_per_scene=views.stop - views.start, sh_degree=self.cfg.sh_eval_degree,
                      check=self.cfg.check_overflow and single, debug=self.cfg.debug)
            if depth_mode is None:
                rgb, _ = rasterize_differentiable(*gauss, c, image_shape, **kw)
                colors.append(rgb)
            else:
                out = rasterize_with_depth_differentiable(*gauss, c, image_shape, near=pick(nr), far=pick(fr),
                                                          depth_mode=depth_mode, color=color, **kw)
                colors.append(out.color)
                depths.append(out.depth)
        if not single and self.cfg.check_overflow:
            check_status(gaussians.means.device)
        return (merge_view_groups(colors, b) if color else None,
                merge_view_groups(depths, b) if depths else None)

    def _render(self, gaussians, extrinsics, intrinsics, near, far, image_shape, depth_mode, color):
        """One rasterizer call over the un-repeated Gaussians for all (b v) views: colour and / or
        the depth render of `depth_mode` from the same pass. More than 32 views per scene: one call
        per group of plan_view_groups, the overflow status checked once after the last."""
        b, v, _, _ = extrinsics.shape
        nr = rearrange(near, "b v -> (b v)")
        fr = rearrange(far, "b v -> (b v)")
        cams = prepare_cameras(
            rearrange(extrinsics, "b v i j -> (b v) i j"),
            rearrange(intrinsics, "b v i j -> (b v) i j"),
            nr,
            fr,
            repeat(self.background_color, "c -> (b v) c", b=b, v=v),
        )
        gauss = (gaussians.means, gaussians.covariances, gaussians.harmonics, gaussians.opacities)
        groups = plan_view_groups(b, v, self.cfg.views_per_call)
        single = len(groups) == 1
        outs = []
        for views in groups:
            pick = lambda t: select_view_rows(t, b, v, views)
            c = cams if single else RasterCameras(*(pick(getattr(cams, f)) for f in cams.__dataclass_fields__))
            kw = dict(views_per_scene=views.stop - views.start, sh_degree=self.cfg.sh_eval_degree,
                      check=self.cfg.check_overflow and single, debug=self.cfg.debug)
            if depth_mode is None:
                rgb, radii = rasterize(*gauss, c, image_shape, **kw)
                outs.append(RasterOutput(rgb, radii, None, None))
            else:
                outs.append(rasterize_with_depth(*gauss, c, image_shape, near=pick(nr), far=pick(fr),
                                                 depth_mode=depth_mode, color=color, **kw))
        if single:
            return outs[0]
        if self.cfg.check_overflow:
            check_status(gaussians.means.device)
        merge = lambda name: (None if getattr(outs[0], name) is None
                              else merge_view_groups([getattr(o, name) for o in outs], b))
        return RasterOutput(merge("color"), merge("radii"), merge("depth"), merge("alpha"))

    def render_depth(
        self,
        gaussians: Gaussians,
        extrinsics: Tensor,
        intrinsics: Tensor,
        near: Tensor,
        far: Tensor,
        image_shape: tuple[int, int],
        mode: DepthRenderingMode = "depth",
    ) -> Tensor:
        """The reference's depth render (render_depth_cuda, cuda_splatting.py:375-417): one
        depth-only rasterizer call for every view (the fake colour is computed per (view, Gaussian)
        in the preprocess kernel). TSPLAT_DEPTH_FUSED=0 keeps the two-pass route: the Gaussians
        repeated per view and rendered with depth_fake_color as their colour. With both differentiable
        flags on and grad wanted the depth carries a grad_fn (the depth-only differentiable call; the
        environment switch governs the forward-only calls alone)."""
        b, v, _, _ = extrinsics.shape
        if self.cfg.differentiable_depth and self._wants_grad(gaussians):
            _, depth = self._render_differentiable(gaussians, extrinsics, intrinsics, near, far, image_shape, mode,
                                                   color=False)
            return rearrange(depth, "(b v) h w -> b v h w", b=b, v=v)
        if _depth_fused():
            out = self._render(gaussians, extrinsics, intrinsics, near, far, image_shape, mode, color=False)
            return rearrange(out.depth, "(b v) h w -> b v h w", b=b, v=v)
        ext = rearrange(extrinsics, "b v i j -> (b v) i j")
        means = repeat(gaussians.means, "b g xyz -> (b v) g xyz", v=v)
        nr = rearrange(near, "b v -> (b v)")
        fr = rearrange(far, "b v -> (b v)")
        fake = depth_fake_color(ext, means, nr, fr, mode)
        cams = prepare_cameras(ext, rearrange(intrinsics, "b v i j -> (b v) i j"), nr, fr,
                               torch.zeros((b * v, 3), device=ext.device))
        color, _ = rasterize(
            means,
            repeat(gaussians.covariances, "b g i j -> (b v) g i j", v=v),
            repeat(fake, "bv g -> bv g c ()", c=3).contiguous(),
            repeat(gaussians.opacities, "b g -> (b v) g", v=v),
            cams,
            image_shape,
            views_per_scene=1,
            sh_degree=0,
            check=self.cfg.check_overflow,
            debug=self.cfg.debug,
        )
        return rearrange(color.mean(dim=1), "(b v) h w -> b v h w", b=b, v=v)

    @staticmethod
    def check_overflow(device) -> None:
        check_status(device)
