"""The scenes of the rasterizer-backward tests and their float64 references, computed once per process and
shared read-only by tests/test_raster_grad_host.py and tests/test_raster_grad.py (TEST INFRASTRUCTURE ONLY).

grad_color is seeded normal noise, set to ZERO on every pixel flagged by the literal oracle
(oracle.raster.render_flagged, any bit) or by the restatement's ambiguity mask, and on the views the
reference does not render: a flagged pixel contributes exactly nothing on both sides."""
from functools import lru_cache

import numpy as np
import torch

import raster_grad_ref
import test_raster_depth as depth_scenes
from oracle import raster as oracle_raster
from transplat_amd import synthetic as S
from transplat_amd.model.decoder.hip_splatting import prepare_cameras

MAX_FLAGGED = depth_scenes.MAX_FLAGGED  # at most 1 % of the pixels flagged
BG = (0.3, 0.3, 0.3)
NAMES = ["tiny", "tiny_deg4", "tiny_s1", "B", "D", "C16"]
SEEDS = {"tiny": 101, "tiny_deg4": 102, "tiny_s1": 103, "B": 104, "D": 105, "C16": 106}


@lru_cache(maxsize=None)
def case(name):
    """-> dict(g: the four Gaussian tensors [S, G, ...] fp32, ext, K, near, far [V...], vps, hw, sh_degree (the
    value handed to rasterize), deg (the degree evaluated), scale_invariant, views (rendered by the reference))"""
    if name.startswith("tiny"):  # 2 scenes x 3 views, G = 1,920, partial tiles in both directions, s = 2
        hw = (24, 40)
        g = S.make_gaussians(2, image_shape=hw)
        ext, K, near, far, vps = depth_scenes._flat_target(S.make_batch(2, image_shape=hw, near=0.5, far=50.0))
        deg = 4 if name == "tiny_deg4" else None
        return dict(g=g, ext=ext, K=K, near=near, far=far, vps=vps, hw=hw, sh_degree=deg, deg=4 if deg else 3,
                    scale_invariant=name != "tiny_s1", views=list(range(6)))
    if name == "C16":  # scene C's 9,000 Gaussians in ONE 16x16 tile: the in-global-memory sort path
        g, ext, K, near, far, vps, _ = depth_scenes.scene("C")
        return dict(g=g, ext=ext, K=K, near=near, far=far, vps=vps, hw=(16, 16), sh_degree=None, deg=3,
                    scale_invariant=True, views=[0])
    g, ext, K, near, far, vps, hw = depth_scenes.scene(name)  # B: near-plane culls; D: 64 exact depths (ties by id)
    return dict(g=g, ext=ext, K=K, near=near, far=far, vps=vps, hw=hw, sh_degree=None, deg=3, scale_invariant=True,
                views=[1] if name == "B" else [0])


ONE_TILE_HW = (8, 16)


def one_tile_case(num_gaussians, scenes=2, vps=2, sh_coeffs=16, seed=0):
    """A seeded scene rendered at H = 8, W = 16 with every Gaussian projected inside the image: ONE tile and two
    live waves (the tile's lower 8 rows are outside the image), each adding at most once per (entry, field). So a
    gradient record receives at most two float atomic adds onto its zero fill, and since IEEE addition of two
    values is commutative the gradients repeat bit for bit between runs: the one place where they do (used by
    tools/raster_bits.py and pinned by test_raster_grad.py). -> (g dict [S, G, ...], ext, K, near, far [S vps])"""
    gen = torch.Generator().manual_seed(7000 + seed)
    rand = lambda *shape: torch.rand(shape, generator=gen)
    s, n, v = scenes, num_gaussians, scenes * vps
    means = torch.stack(((rand(s, n) - 0.5) * 2.0, (rand(s, n) - 0.5) * 2.0, 3.5 + rand(s, n)), dim=-1)
    a = (rand(s, n, 3, 3) - 0.5) * 0.3
    cov = a @ a.transpose(-1, -2) + 0.002 * torch.eye(3)
    sh = torch.randn((s, n, 3, sh_coeffs), generator=gen) * 0.3
    op = 0.01 + rand(s, n) * min(0.6, 60.0 / n)
    ext = torch.eye(4).repeat(v, 1, 1)
    ext[:, 0, 3] = (rand(v) - 0.5) * 0.1  # the views differ by a small shift; scale s = 1 and 2 alternate
    near = torch.tensor([1.0, 0.5]).repeat(v)[:v].contiguous()
    g = {"means": means, "covariances": cov.contiguous(), "harmonics": sh, "opacities": op}
    return g, ext, S.intrinsics(v), near, torch.full((v,), 100.0)


def cameras(name, device="cpu"):
    c = case(name)
    d = lambda t: t.to(device)
    v = c["ext"].shape[0]
    return prepare_cameras(d(c["ext"]), d(c["K"]), d(c["near"]), d(c["far"]), d(torch.tensor(BG).expand(v, 3).contiguous()),
                           scale_invariant=c["scale_invariant"])


@lru_cache(maxsize=None)
def reference(name):
    """-> dict(color [V, 3, H, W] float64 (views of case()['views']; 0 elsewhere), oracle_color, flagged [V, H, W]
    bool (oracle or restatement; True on the views not rendered), flagged_fraction (over the rendered views), kinks,
    radii, oracle_radii, grad_color [V, 3, H, W] fp32 (0 where flagged), grads: the four float64 gradients)"""
    c = case(name)
    g, hw, vps, deg = c["g"], c["hw"], c["vps"], c["deg"]
    cams = cameras(name)
    args = (g["means"], g["covariances"], g["harmonics"], g["opacities"], cams, hw, vps, deg)
    o_color, o_radii, _, pflag, _ = oracle_raster.render_flagged(*args)
    first = raster_grad_ref.render(*args, views=c["views"])
    v = c["ext"].shape[0]
    rendered = torch.zeros(v, dtype=torch.bool)
    rendered[c["views"]] = True
    flagged = torch.from_numpy(pflag != 0) | first["ambiguous"] | ~rendered[:, None, None]
    gen = torch.Generator().manual_seed(SEEDS[name])
    grad_color = torch.randn((v, 3, *hw), generator=gen)
    grad_color = torch.where(flagged[:, None], torch.zeros(()), grad_color).contiguous()
    out = raster_grad_ref.render(*args, grad_color=grad_color, views=c["views"], frozen=first["decisions"])
    n_flag = int(flagged[rendered].sum())
    return dict(color=first["color"], oracle_color=torch.from_numpy(np.asarray(o_color)), flagged=flagged,
                flagged_fraction=n_flag / float(rendered.sum() * hw[0] * hw[1]), kinks=first["kinks"],
                radii=first["radii"], oracle_radii=torch.from_numpy(np.asarray(o_radii)), grad_color=grad_color,
                grads=out["grads"], rendered=rendered)
