"""Float64 yardstick of the fused colour + depth + alpha backward (tsplat_raster_depth_bwd), composed from what
exists (TEST INFRASTRUCTURE ONLY): tests/test_raster_depth_grad_host.py and tests/test_raster_depth_grad.py.

F : (means, covariances, harmonics, opacities) -> (color, depth, alpha) of tsplat_raster_depth_fwd is three
renders of tests/raster_grad_ref.py, which is the reference's own definition of the depth render
(render_depth_cuda): per view,
  * the colour render, as tests/raster_grad_cases.py runs it;
  * the same render over a black background with the degree-0 harmonic f(z(means)), f the mode's fake colour,
    built in float64 by decoder_splatting_hip.depth_fake_color from the UNSCALED extrinsics; its channel mean is
    the depth;
  * the same render with the constant harmonic 0.5 / C0 (colour 1): its channel mean is alpha.
All three share ONE set of frozen decisions (those of the colour render), so autograd differentiates the sum
of the three seeded losses with every discrete decision held fixed. No new blend code.

Seeds: grad_color is tests/raster_grad_cases.py's; grad_depth and grad_alpha are seeded normal noise, zero on
every pixel flagged by the oracle or by the restatement's ambiguity mask and on the views not rendered.
Conditions the tests assert (they are not tolerances): flagged share <= MAX_FLAGGED, no kink of the colour
render, and no visible Gaussian with |C0 f + 0.5| < 1e-5 (the depth render's own kink count: its "colour" IS
C0 f + 0.5).

`variant`: None: the cameras' planes go to the render; "clamp": near x 4 (relative_disparity then clamps a
share of the Gaussians at 0); "swap": near and far exchanged (log mode's pass branch far < z < near).
"""
from functools import lru_cache

import torch

import raster_grad_cases as cases
import raster_grad_ref
from transplat_amd.model.decoder.decoder_splatting_hip import depth_fake_color
from transplat_amd.model.decoder.hip_splatting import RasterCameras

C0 = raster_grad_ref.C0
CLAMP_EPS = raster_grad_ref.KINK_EPS  # 1e-5
KINDS = ("means", "covariances", "harmonics", "opacities")
SEED_OFFSET = 1000


def planes(name, variant=None):
    """-> (near [V], far [V]) fp32 as handed to the depth render (not to prepare_cameras)."""
    c = cases.case(name)
    near, far = c["near"].clone(), c["far"].clone()
    if variant == "clamp":
        near = near * 4
    elif variant == "swap":
        near, far = far, near
    elif variant is not None:
        raise KeyError(variant)
    return near, far


@lru_cache(maxsize=None)
def base(name):
    """The colour render's decisions (shared by the three renders), the flags and the extra seeds of a scene."""
    c = cases.case(name)
    ref = cases.reference(name)
    g, hw = c["g"], c["hw"]
    cams = cases.cameras(name)
    first = raster_grad_ref.render(g["means"], g["covariances"], g["harmonics"], g["opacities"], cams, hw, c["vps"],
                                   c["deg"], views=c["views"])
    flagged = ref["flagged"] | first["ambiguous"]
    gen = torch.Generator().manual_seed(cases.SEEDS[name] + SEED_OFFSET)
    v = c["ext"].shape[0]
    seed = lambda: torch.where(flagged, torch.zeros(()), torch.randn((v, *hw), generator=gen)).contiguous()
    grad_depth, grad_alpha = seed(), seed()
    rendered = ref["rendered"]
    return dict(decisions=first["decisions"], flagged=flagged, kinks=first["kinks"], grad_color=ref["grad_color"],
                grad_depth=grad_depth, grad_alpha=grad_alpha, rendered=rendered,
                flagged_fraction=int(flagged[rendered].sum()) / float(rendered.sum() * hw[0] * hw[1]))


def _black(cams):
    return RasterCameras(cams.viewmat, cams.projmat, cams.campos, cams.tanfov, torch.zeros_like(cams.bg), cams.scale)


@lru_cache(maxsize=None)
def reference(name, mode, variant=None, parts=("color", "depth", "alpha")):
    """-> dict(grads: the four float64 gradients of sum(color gc) + sum(depth gd) + sum(alpha ga) over `parts`;
    color / depth / alpha: the float64 renders ([V, 3, H, W], [V, H, W], [V, H, W]; 0 on the views not rendered);
    the seeds; kinks (colour render), depth_kinks (visible Gaussians with |C0 f + 0.5| < 1e-5, or at the tx / ty
    clamp); visible, clamped (C0 f + 0.5 <= 0), log_inside (far < z < near strictly): counts over the visible
    (view, Gaussian) pairs of the rendered views)"""
    c = cases.case(name)
    b = base(name)
    g, hw, vps, deg = c["g"], c["hw"], c["vps"], c["deg"]
    cams = cases.cameras(name)
    dark = _black(cams)
    near, far = (t.double() for t in planes(name, variant))
    ext = c["ext"].double()
    leaves = [g[k].double().clone().requires_grad_() for k in KINDS]
    means = leaves[0]
    s, n = means.shape[:2]
    v_total = ext.shape[0]
    out = {k: torch.zeros((v_total, *(([3] if k == "color" else []) + list(hw))), dtype=torch.float64)
           for k in ("color", "depth", "alpha")}
    grads = [torch.zeros_like(t) for t in leaves]
    one = torch.full((s, n, 3, 1), 0.5 / C0, dtype=torch.float64)
    seeds = {"color": b["grad_color"].double(), "depth": b["grad_depth"].double(), "alpha": b["grad_alpha"].double()}
    depth_kinks = visible = clamped = log_inside = 0
    for v in c["views"]:
        sc = v // vps
        render = lambda sh, cam, d: raster_grad_ref.render(means, leaves[1], sh, leaves[3], cam, hw, vps, d, views=[v],
                                                           frozen=b["decisions"], create_graph=True)
        fake = depth_fake_color(ext[v:v + 1], means[sc][None], near[v:v + 1], far[v:v + 1], mode)[0]  # [G]
        ok = b["decisions"][v]["ok"]
        with torch.no_grad():
            raw = C0 * fake[ok] + 0.5
            z = depth_fake_color(ext[v:v + 1], means[sc][None], near[v:v + 1], far[v:v + 1], "depth")[0][ok]
            visible += int(ok.sum())
            clamped += int((raw <= 0).sum())
            log_inside += int(((z > far[v]) & (z < near[v])).sum())
        loss = 0.0
        if "color" in parts:
            col = render(leaves[2], cams, deg)["color"][v]
            out["color"][v] = col.detach()
            loss = loss + (col * seeds["color"][v]).sum()
        if "depth" in parts:
            r = render(fake[None, :, None, None].expand(s, n, 3, 1), dark, 0)
            depth_kinks += r["kinks"]
            dep = r["color"][v].mean(dim=0)
            out["depth"][v] = dep.detach()
            loss = loss + (dep * seeds["depth"][v]).sum()
        if "alpha" in parts:
            alp = render(one, dark, 0)["color"][v].mean(dim=0)
            out["alpha"][v] = alp.detach()
            loss = loss + (alp * seeds["alpha"][v]).sum()
        for acc, gr in zip(grads, torch.autograd.grad(loss, leaves, allow_unused=True)):
            if gr is not None:
                acc += gr
    return dict(grads=tuple(grads), **out, grad_color=b["grad_color"], grad_depth=b["grad_depth"],
                grad_alpha=b["grad_alpha"], flagged=b["flagged"], flagged_fraction=b["flagged_fraction"],
                kinks=b["kinks"], depth_kinks=depth_kinks, visible=visible, clamped=clamped, log_inside=log_inside,
                rendered=b["rendered"])


def check_conditions(ref):
    """The asserted conditions of the yardstick (module docstring)."""
    assert ref["flagged_fraction"] <= cases.MAX_FLAGGED, ref["flagged_fraction"]
    assert ref["kinks"] == 0 and ref["depth_kinks"] == 0, (ref["kinks"], ref["depth_kinks"])
