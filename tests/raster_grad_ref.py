"""Float64 restatement of the colour render F of tsplat_raster_fwd, differentiated by autograd: the
yardstick of tests/test_raster_grad.py and tests/test_raster_grad_host.py (TEST INFRASTRUCTURE ONLY).

F : (means [S, G, 3], covariances [S, G, 3, 3], harmonics [S, G, 3, M], opacities [S, G]) -> color
[V, 3, H, W], cameras, background, scale and sh_degree fixed. The restatement takes the fp32 inputs
promoted to double and makes every discrete decision of the forward itself, in float64: the near-plane
cull vz > 0.2, det != 0, the radius and the 16x16 tile rectangle, the (depth, id) order, power > 0,
alpha < 1/255 and test_T < 1e-4. The decisions are taken on detached values and enter the
differentiable part as masks and index lists, so autograd differentiates F with the decisions held
fixed; the piecewise rules (colour clamp at 0, alpha cap at 0.99, the +-1.3 tan(fov) clamp of vx / tz
and vy / tz as a function of both, upper-triangle covariance entries only) are torch.clamp /
torch.minimum / indexing and differentiate as written.

Dense per tile: [tile list x 256 pixels], the tile list being the Gaussians whose rectangle covers the
tile, as in the forward. `render()` returns the colour, the four gradients for a grad_color, a per-pixel
ambiguity mask and a count of Gaussian-level kinks:
  * mask: a pixel where two entries of one order-ambiguous group both contribute (entries adjacent in
    the tile's order whose float64 depths differ by less than 1e-6 relative but are not equal: the
    kernel's fp32 order may differ; equal depths are ordered by id on both sides, and a pair whose
    fp32 depths are both exact -- the kernel's depth expression evaluated in fp32 equals the float64
    value, as under an identity camera with a power-of-two scale -- has the float64 order in fp32
    too, so it is not ambiguous however close the depths), or where
    o e^power of a contributing entry lies within 1e-5 of 0.99;
  * kinks: a colour channel of a rendered (view, Gaussian) within 1e-5 of the clamp at 0, or
    vx / tz, vy / tz within 1e-5 relative of +-1.3 tan(fov).
`frozen`: the decisions of an earlier call, used instead of recomputing them (gradcheck of the smooth
core: a finite-difference step must not flip a decision).
"""
from __future__ import annotations

import math

import torch

TILE = 16
ORDER_EPS = 1e-6
ALPHA_EPS = 1e-5
KINK_EPS = 1e-5

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435]
C4 = [2.5033429417967046, -1.7701307697799304, 0.9461746957575601, -0.6690465435572892, 0.10578554691520431,
      -0.6690465435572892, 0.47308734787878004, -1.7701307697799304, 0.6258357354491761]


def sh_basis(d: torch.Tensor, deg: int) -> torch.Tensor:
    """d [G, 3] (not normalised) -> the (deg + 1)^2 real SH basis values [G, K], the rasterizer's signs."""
    n = d / d.norm(dim=-1, keepdim=True)
    x, y, z = n.unbind(-1)
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    b = [torch.full_like(x, C0)]
    if deg > 0:
        b += [-C1 * y, C1 * z, -C1 * x]
    if deg > 1:
        b += [C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if deg > 2:
        b += [C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy),
              C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
              C3[6] * x * (xx - 3 * yy)]
    if deg > 3:
        b += [C4[0] * xy * (xx - yy), C4[1] * yz * (3 * xx - yy), C4[2] * xy * (7 * zz - 1),
              C4[3] * yz * (7 * zz - 3), C4[4] * (zz * (35 * zz - 30) + 3), C4[5] * xz * (7 * zz - 3),
              C4[6] * (xx - yy) * (7 * zz - 1), C4[7] * xz * (xx - 3 * yy),
              C4[8] * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(b, -1)


def _preprocess(means, cov, sh, op, cam, hw, deg):
    """One view. cam: dict of float64 tensors (viewmat [16], projmat [16], campos [3], tanfov [2], scale [2]).
    -> differentiable per-Gaussian (px, py, conic a b c, rgb [G, 3], opacity, depth) + (ok, radius, kinks)."""
    h, w = hw
    vm, pm, s, s2 = cam["viewmat"], cam["projmat"], cam["scale"][0], cam["scale"][1]
    m = means * s
    mx, my, mz = m.unbind(-1)
    vx = vm[0] * mx + vm[4] * my + vm[8] * mz + vm[12]
    vy = vm[1] * mx + vm[5] * my + vm[9] * mz + vm[13]
    vz = vm[2] * mx + vm[6] * my + vm[10] * mz + vm[14]
    ok = vz.detach() > 0.2
    # the depth as the kernel's fp32 expression gives it (separately rounded products and sums, in order);
    # where it EQUALS the float64 depth the kernel's sort key is exact and cannot be misordered
    with torch.no_grad():
        f32 = lambda t: t.detach().to(torch.float32)
        m32 = f32(means) * f32(s)
        v32 = f32(vm)
        d32 = v32[2] * m32[:, 0] + v32[6] * m32[:, 1] + v32[10] * m32[:, 2] + v32[14]
        depth_exact = d32.to(torch.float64) == vz.detach()
    vz_safe = torch.where(ok, vz, torch.ones_like(vz))  # culled rows stay finite; they are never used
    hx = pm[0] * mx + pm[4] * my + pm[8] * mz + pm[12]
    hy = pm[1] * mx + pm[5] * my + pm[9] * mz + pm[13]
    hwc = pm[3] * mx + pm[7] * my + pm[11] * mz + pm[15]
    pw = 1.0 / (hwc + 0.0000001)
    px = ((hx * pw + 1.0) * w - 1.0) * 0.5
    py = ((hy * pw + 1.0) * h - 1.0) * 0.5
    # the six upper-triangle entries, as the kernel reads them
    k = cov * s2
    c00, c01, c02, c11, c12, c22 = k[:, 0, 0], k[:, 0, 1], k[:, 0, 2], k[:, 1, 1], k[:, 1, 2], k[:, 2, 2]
    tfx, tfy = cam["tanfov"][0], cam["tanfov"][1]
    fx, fy = w / (2.0 * tfx), h / (2.0 * tfy)
    limx, limy = 1.3 * tfx, 1.3 * tfy
    tz = vz_safe
    rxu, ryu = vx / tz, vy / tz
    tx = torch.minimum(limx, torch.maximum(-limx, rxu)) * tz
    ty = torch.minimum(limy, torch.maximum(-limy, ryu)) * tz
    j00, j02 = fx / tz, -(fx * tx) / (tz * tz)
    j11, j12 = fy / tz, -(fy * ty) / (tz * tz)
    n0 = [j00 * vm[0] + j02 * vm[2], j00 * vm[4] + j02 * vm[6], j00 * vm[8] + j02 * vm[10]]
    n1 = [j11 * vm[1] + j12 * vm[2], j11 * vm[5] + j12 * vm[6], j11 * vm[9] + j12 * vm[10]]
    cm = [[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]]
    quad = lambda p, q: sum(p[i] * cm[i][j] * q[j] for i in range(3) for j in range(3))
    a = quad(n0, n0) + 0.3
    b = quad(n0, n1)
    c = quad(n1, n1) + 0.3
    det = a * c - b * b
    ok = ok & (det.detach() != 0)
    det_safe = torch.where(ok, det, torch.ones_like(det))
    qa, qb, qc = c / det_safe, -b / det_safe, a / det_safe
    mid = 0.5 * (a + c)
    root = torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    radius = torch.ceil(3.0 * torch.sqrt(torch.maximum(mid + root, mid - root))).detach().to(torch.int64)
    basis = sh_basis(m - cam["campos"], deg)  # [G, K]
    raw = (sh[:, :, : basis.shape[-1]] * basis[:, None, :]).sum(-1) + 0.5  # [G, 3]
    rgb = torch.clamp(raw, min=0.0)
    kinks = ((raw.detach().abs() < KINK_EPS).any(-1)
             | ((rxu.detach().abs() - limx).abs() < KINK_EPS * limx)
             | ((ryu.detach().abs() - limy).abs() < KINK_EPS * limy))
    return dict(px=px, py=py, qa=qa, qb=qb, qc=qc, rgb=rgb, op=op, depth=vz, depth_exact=depth_exact, ok=ok,
                radius=radius, kinks=kinks)


def _rects(px, py, radius, ok, hw):
    """getRect of the reference: (int) truncation, clamped to the tile grid -> x0, y0, x1, y1 and the final ok."""
    h, w = hw
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    r = radius.to(torch.float64)
    tr = lambda t, hi: torch.clamp(torch.trunc(t).to(torch.int64), 0, hi)
    x0, y0 = tr((px - r) / TILE, tx), tr((py - r) / TILE, ty)
    x1, y1 = tr((px + r + (TILE - 1)) / TILE, tx), tr((py + r + (TILE - 1)) / TILE, ty)
    ok = ok & ((x1 - x0) * (y1 - y0) != 0)
    return x0, y0, x1, y1, ok


def _view_decisions(pre, hw):
    h, w = hw
    px, py = pre["px"].detach(), pre["py"].detach()
    finite = torch.isfinite(px) & torch.isfinite(py)
    px, py = torch.where(finite, px, torch.zeros_like(px)), torch.where(finite, py, torch.zeros_like(py))
    x0, y0, x1, y1, ok = _rects(px, py, pre["radius"], pre["ok"] & finite, hw)
    depth = pre["depth"].detach()
    order = torch.sort(depth, stable=True).indices  # (depth, id): stable over id-ordered rows
    order = order[ok[order]]
    tiles = {}
    for ty in range((h + TILE - 1) // TILE):
        for tx in range((w + TILE - 1) // TILE):
            cover = (x0[order] <= tx) & (tx < x1[order]) & (y0[order] <= ty) & (ty < y1[order])
            tiles[(tx, ty)] = {"idx": order[cover]}
    return {"ok": ok, "tiles": tiles}


def _blend_tile(pre, idx, tx, ty, hw, bg, dec):
    """-> colour [3, P] of the tile's in-image pixels (row-major in the tile), ambiguity mask [P], pixel coords."""
    h, w = hw
    ys = torch.arange(ty * TILE, min((ty + 1) * TILE, h), dtype=torch.float64)
    xs = torch.arange(tx * TILE, min((tx + 1) * TILE, w), dtype=torch.float64)
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    n, npix = idx.numel(), gx.numel()
    if n == 0:
        return bg[:, None].expand(3, npix), torch.zeros(npix, dtype=torch.bool), gx, gy
    dx = pre["px"][idx, None] - gx[None, :]
    dy = pre["py"][idx, None] - gy[None, :]
    power = -0.5 * (pre["qa"][idx, None] * dx * dx + pre["qc"][idx, None] * dy * dy) - pre["qb"][idx, None] * dx * dy
    o = pre["op"][idx, None]
    if "contrib" in dec:
        contrib, acc = dec["contrib"], dec["acc"]
    else:
        pd = power.detach()
        raw_d = o.detach() * torch.exp(torch.clamp(pd, max=0.0))
        contrib = ~(pd > 0) & ~(torch.clamp(raw_d, max=0.99) < 1.0 / 255.0)
        a_d = torch.where(contrib, torch.clamp(raw_d, max=0.99), torch.zeros_like(raw_d))
        test_t = torch.cumprod(1.0 - a_d, dim=0)  # T after the entry, were it accumulated
        acc = contrib & ~(test_t < 0.0001)
        dec["contrib"], dec["acc"] = contrib, acc
        # entries the walk evaluates with an effect: accumulated ones and the one that stops the pixel
        t_before = torch.cat([torch.ones_like(test_t[:1]), test_t[:-1]], 0)
        live = contrib & ~(t_before < 0.0001)
        depth = pre["depth"].detach()[idx]
        gap = (depth[1:] - depth[:-1]).abs()
        exact = pre["depth_exact"][idx]
        amb_next = (gap > 0) & (gap < ORDER_EPS * depth[1:].abs()) & ~(exact[1:] & exact[:-1])
        group = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum((~amb_next).to(torch.int64), 0)])
        gl = torch.where(live, group[:, None], torch.full_like(group[:, None], -1))
        prev = torch.cat([torch.full_like(gl[:1], -1), torch.cummax(gl, dim=0).values[:-1]], 0)
        dec["amb"] = ((live & (prev == group[:, None])).any(0)
                      | (live & ((raw_d - 0.99).abs() < ALPHA_EPS)).any(0))
    raw = o * torch.exp(torch.where(acc, power, torch.zeros_like(power)))
    alpha = torch.where(acc, torch.clamp(raw, max=0.99), torch.zeros_like(raw))
    one_minus = 1.0 - alpha
    t_incl = torch.cumprod(one_minus, dim=0)
    t_excl = torch.cat([torch.ones_like(t_incl[:1]), t_incl[:-1]], 0)
    wgt = alpha * t_excl  # [n, P]
    color = torch.einsum("np,nc->cp", wgt, pre["rgb"][idx]) + t_incl[-1][None, :] * bg[:, None]
    return color, dec.get("amb", torch.zeros(npix, dtype=torch.bool)), gx, gy


def render(means, covariances, harmonics, opacities, cams, image_shape, views_per_scene, sh_degree,
           grad_color=None, views=None, frozen=None, create_graph=False):
    """Inputs in the tsplat_raster_fwd layouts (any float dtype, promoted to float64; cams: a
    RasterCameras of host tensors). `views`: the views to render (default all; the others stay 0).
    -> dict(color [V, 3, H, W] float64, grads (means, covariances, harmonics, opacities) for
    grad_color [V, 3, H, W] or None, ambiguous [V, H, W] bool, kinks int, radii [V, G] int64,
    decisions (pass as `frozen` to hold them)). With create_graph the colour keeps its graph and the
    inputs are used as given (gradcheck)."""
    h, w = image_shape
    f64 = lambda t: torch.as_tensor(t).to(torch.float64)
    if create_graph:
        leaves = [means, covariances, harmonics, opacities]
    else:
        leaves = [f64(t).detach().clone().requires_grad_(grad_color is not None)
                  for t in (means, covariances, harmonics, opacities)]
    mean_l, cov_l, sh_l, op_l = leaves
    v_total = cams.viewmat.shape[0]
    g = mean_l.shape[1]
    color = torch.zeros((v_total, 3, h, w), dtype=torch.float64)
    amb = torch.zeros((v_total, h, w), dtype=torch.bool)
    radii = torch.zeros((v_total, g), dtype=torch.int64)
    kinks = 0
    decisions = {} if frozen is None else frozen
    gc = None if grad_color is None else f64(grad_color)
    grads = [torch.zeros_like(t) for t in leaves] if gc is not None else None
    for v in (range(v_total) if views is None else views):
        sc = v // views_per_scene
        cam = {k: f64(getattr(cams, k)[v]) for k in ("viewmat", "projmat", "campos", "tanfov", "scale")}
        bg = f64(cams.bg[v])
        pre = _preprocess(mean_l[sc], cov_l[sc], sh_l[sc], op_l[sc], cam, (h, w), sh_degree)
        if v not in decisions:
            decisions[v] = _view_decisions(pre, (h, w))
        dec = decisions[v]
        radii[v] = torch.where(dec["ok"], pre["radius"], torch.zeros_like(pre["radius"]))
        kinks += int((pre["kinks"] & dec["ok"]).sum())
        loss = 0.0
        for (tx, ty), td in dec["tiles"].items():
            col, am, gx, gy = _blend_tile(pre, td["idx"], tx, ty, (h, w), bg, td)
            ix, iy = gx.to(torch.int64), gy.to(torch.int64)
            color[v][:, iy, ix] = col if create_graph else col.detach()
            amb[v][iy, ix] = am
            if gc is not None:
                loss = loss + (col * gc[v][:, iy, ix]).sum()
        if gc is not None and torch.is_tensor(loss) and loss.requires_grad:
            for acc_g, gr in zip(grads, torch.autograd.grad(loss, leaves, allow_unused=True)):
                if gr is not None:
                    acc_g += gr
    return {"color": color, "grads": None if grads is None else tuple(grads), "ambiguous": amb, "kinks": kinks,
            "radii": radii, "decisions": decisions}
