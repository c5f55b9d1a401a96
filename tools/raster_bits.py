"""One sha256 of the output bytes per rasterizer case, for comparing two builds of the library bit for bit
(TSPLAT_LIB points at the other build).

Forward cases (colour, depth, alpha, radii): the scenes of the raster tests -- raster_grad_cases.NAMES, the
test_raster_depth scenes in each of their modes (A also without scale invariance), and the scenes of
tests/test_raster.py, the 1216 x 1216 image, the G = 589,824 stress scene and the graph-replay scenes included (its
GPU tests build them inline; restated here with the same generator calls, but for the saturation scene, whose
colours the test draws from the unseeded global generator and this tool from a seeded one) -- each under the default tile sort and TSPLAT_RASTER_SORT=bitonic,
through rasterize, rasterize_with_depth with colour + depth + alpha, and depth only with color=False.

Backward cases (the four gradient tensors): gradients are float atomic sums and in general do not repeat; they do on
raster_grad_cases.one_tile_case scenes (H = 8, W = 16: at most two adds per record field). G = 40 (register bitonic
sort), 600 (counting sort), 5,000 (above the LDS sort's capacity: the global path), 2 scenes x 2 views, (M, degree) in
(25, 4), (16, 3), (9, 1); through tsplat_raster_bwd, the depth backward with colour + depth + alpha seeds in each depth
mode, and with depth + alpha seeds and no colour gradient. Run the tool twice on one build first: a case that differs
between those two runs does not repeat and says nothing about two builds.

usage: [TSPLAT_LIB=other.so] python tools/raster_bits.py out.json
       python tools/raster_bits.py --compare a.json b.json"""
import hashlib
import json
import os
import sys
from pathlib import Path

if sys.argv[1:2] == ["--compare"]:
    a, b = (json.loads(Path(p).read_text()) for p in sys.argv[2:4])
    differ = sorted(k for k in a.keys() | b.keys() if a.get(k) != b.get(k))
    print(f"{sys.argv[2]} vs {sys.argv[3]}: {len(a)} and {len(b)} cases, {len(differ)} differ")
    print("".join(f"  {k}\n" for k in differ), end="")
    sys.exit(1 if differ else 0)

import torch  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import raster_grad_cases as cases  # noqa: E402
import test_raster_depth as depth_scenes  # noqa: E402
from transplat_amd import synthetic as S  # noqa: E402
from transplat_amd.model.decoder.hip_splatting import (prepare_cameras, rasterize, rasterize_differentiable,  # noqa: E402
                                                       rasterize_with_depth, rasterize_with_depth_differentiable)

dev = torch.device("cuda:0")
MODES = depth_scenes.MODES
KINDS = ("means", "covariances", "harmonics", "opacities")
out = {}


def put(tag, **tensors):
    h = hashlib.sha256()
    for name in sorted(tensors):
        if tensors[name] is not None:
            h.update(name.encode() + tensors[name].detach().contiguous().cpu().numpy().tobytes())
    out[tag] = h.hexdigest()


def d(t):
    return t.to(dev)


def forward_scenes():
    """-> (tag, g, ext, K, near, far, bg, vps, hw, sh_degree, scale_invariant, modes)"""
    for name in cases.NAMES:
        c = cases.case(name)
        bg = torch.tensor(cases.BG).expand(c["ext"].shape[0], 3).contiguous()
        yield (f"grad_cases {name}", c["g"], c["ext"], c["K"], c["near"], c["far"], bg, c["vps"], c["hw"],
               c["sh_degree"], c["scale_invariant"], MODES if name == "tiny" else ["depth"])
    for name in "ABCD":
        g, ext, K, near, far, vps, hw = depth_scenes.scene(name)
        yield (f"depth_scenes {name}", g, ext, K, near, far, torch.zeros(ext.shape[0], 3), vps, hw, None, True,
               MODES if name in "AB" else ["depth"])
    g, ext, K, near, far, vps, hw = depth_scenes.scene("A")  # test_fused_depth_parity_without_scale_invariance
    yield ("depth_scenes A s=1", g, ext, K, near, far, torch.zeros(ext.shape[0], 3), vps, hw, None, False,
           ["relative_disparity"])
    # tests/test_raster.py (near_plane_and_behind_camera is depth_scenes B, long_tile_lists is C, 'ties' is D;
    # capacity_overflow renders nothing; cameras_kernel has no Gaussians)
    target = lambda b, hw, **kw: depth_scenes._flat_target(S.make_batch(b, image_shape=hw, **kw))
    for deg in (3, 4, 0):
        ext, K, near, far, vps = target(1, (64, 64))
        yield (f"test_raster small deg{deg}", S.make_gaussians(1, image_shape=(64, 64)), ext, K, near, far,
               torch.zeros(3, 3), vps, (64, 64), deg, True, ["depth"])
    for offset in (5, 9):  # graph_replay_with_new_inputs (offset 0 is the small scene above)
        ext, K, near, far, vps = target(1, (64, 64))
        yield (f"test_raster graph_replay offset{offset}", S.make_gaussians(1, image_shape=(64, 64), scene_offset=offset),
               ext, K, near, far, torch.zeros(3, 3), vps, (64, 64), None, True, ["depth"])
    ext, K, near, far, vps = target(1, (1216, 1216), num_target=1)  # 5,776 tiles: scatter LDS beyond 64 KB
    yield ("test_raster large_image", S.make_gaussians(1, image_shape=(128, 128)), ext, K, near, far,
           torch.zeros(1, 3), vps, (1216, 1216), 3, True, ["depth"])
    ext, K, near, far, vps = target(1, (384, 512), num_context=3, num_target=1)  # 32 x 24 tiles, G = 589,824
    yield ("test_raster dtu_stress", S.make_gaussians(1, num_context=3, image_shape=(384, 512)), ext, K, near, far,
           torch.zeros(1, 3), vps, (384, 512), 3, True, ["depth"])
    ext, K, near, far, vps = target(3, (48, 80))
    yield ("test_raster multi_scene", S.make_gaussians(3, image_shape=(48, 80)), ext, K, near, far,
           torch.tensor((0.3, 0.6, 0.9)).expand(9, 3).contiguous(), vps, (48, 80), 3, True, ["depth"])
    ext, K, near, far, vps = target(1, (256, 256))
    yield ("test_raster full_size", S.make_gaussians(1, image_shape=(256, 256)), ext, K, near, far, torch.zeros(3, 3),
           vps, (256, 256), 3, True, ["depth"])
    ident = (torch.eye(4)[None], S.intrinsics(1), torch.ones(1), torch.full((1,), 100.0))
    for depths in ("one_depth", "two_clusters"):
        n = 2500
        gen = torch.Generator().manual_seed(11)
        means = torch.zeros((1, n, 3))
        means[0, :, 0] = (torch.rand(n, generator=gen) - 0.5) * 0.3
        means[0, :, 1] = (torch.rand(n, generator=gen) - 0.5) * 0.3
        if depths == "one_depth":
            z = torch.full((n,), 4.0)
        else:
            z = torch.where(torch.rand(n, generator=gen) < 0.5, torch.tensor(4.0),
                            torch.nextafter(torch.tensor(4.0), torch.tensor(5.0)))
            z[: n // 10] = 3.0 + torch.rand(n // 10, generator=gen) * 5.0
        means[0, :, 2] = z
        g = {"means": means, "covariances": (torch.eye(3) * 4e-4).expand(1, n, 3, 3).clone(),
             "harmonics": torch.randn((1, n, 3, 16), generator=gen) * S.sh_mask(3),
             "opacities": 0.05 + torch.rand((1, n), generator=gen) * 0.2}
        yield (f"test_raster {depths}", g, *ident, torch.zeros(1, 3), 1, (64, 64), 3, True, ["depth"])
    n = 64
    means = torch.zeros((1, n, 3))
    means[0, :, 2] = torch.linspace(2, 6, n)
    gen = torch.Generator().manual_seed(13)
    g = {"means": means, "covariances": (torch.eye(3) * 0.5).expand(1, n, 3, 3).clone(),
         "harmonics": torch.rand((1, n, 3, 1), generator=gen) * 2, "opacities": torch.ones((1, n))}
    yield ("test_raster saturation", g, *ident, torch.full((1, 3), 0.5), 1, (32, 32), 0, True, ["depth"])


def forward_cases():
    for tag, g, ext, K, near, far, bg, vps, hw, deg, si, modes in forward_scenes():
        cams = prepare_cameras(d(ext), d(K), d(near), d(far), d(bg), scale_invariant=si)
        args = (d(g["means"]), d(g["covariances"]), d(g["harmonics"]), d(g["opacities"]), cams, hw, vps)
        for sort in ("count", "bitonic"):
            os.environ.pop("TSPLAT_RASTER_SORT", None)
            if sort == "bitonic":
                os.environ["TSPLAT_RASTER_SORT"] = "bitonic"
            color, radii = rasterize(*args, sh_degree=deg)
            put(f"fwd {tag} {sort} rasterize", color=color, radii=radii)
            for mode in modes:
                kw = dict(sh_degree=deg, near=d(near), far=d(far), depth_mode=mode)
                o = rasterize_with_depth(*args, **kw, color=True, alpha=True)
                put(f"fwd {tag} {sort} {mode} all", color=o.color, depth=o.depth, alpha=o.alpha, radii=o.radii)
                o = rasterize_with_depth(*args, **kw, color=False, alpha=False)
                put(f"fwd {tag} {sort} {mode} depth_only", depth=o.depth, radii=o.radii)
    os.environ.pop("TSPLAT_RASTER_SORT", None)


def backward_cases():
    hw = cases.ONE_TILE_HW
    for n in (40, 600, 5000):
        for m, deg in ((25, 4), (16, 3), (9, 1)):
            g, ext, K, near, far = cases.one_tile_case(n, scenes=2, vps=2, sh_coeffs=m, seed=n + m)
            v = ext.shape[0]
            cams = prepare_cameras(d(ext), d(K), d(near), d(far), d(torch.tensor(cases.BG).expand(v, 3).contiguous()))
            gen = torch.Generator().manual_seed(n * 100 + m)
            seeds = {"color": d(torch.randn((v, 3, *hw), generator=gen)), "depth": d(torch.randn((v, *hw), generator=gen)),
                     "alpha": d(torch.randn((v, *hw), generator=gen))}

            def run(tag, parts, fn, **kw):
                t = {k: d(g[k]).clone().requires_grad_(True) for k in KINDS}
                o = fn(t["means"], t["covariances"], t["harmonics"], t["opacities"], cams, hw, 2, sh_degree=deg, **kw)
                outs = {"color": o[0]} if isinstance(o, tuple) else {k: getattr(o, k) for k in parts}
                torch.autograd.backward([outs[k] for k in parts], [seeds[k] for k in parts])
                put(f"bwd G={n} M={m} deg={deg} {tag}", **{k: t[k].grad for k in KINDS})

            run("colour", ("color",), rasterize_differentiable)
            depth_kw = lambda mode: dict(near=d(near), far=d(far), depth_mode=mode, color=True, alpha=True)
            for mode in MODES:
                run(f"{mode} colour+depth+alpha", ("color", "depth", "alpha"), rasterize_with_depth_differentiable,
                    **depth_kw(mode))
            run("depth depth+alpha", ("depth", "alpha"), rasterize_with_depth_differentiable, **depth_kw("depth"))


forward_cases()
backward_cases()
torch.cuda.synchronize()
Path(sys.argv[1]).write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
print(f"{len(out)} cases -> {sys.argv[1]}")
