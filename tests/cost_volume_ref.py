"""The plane-sweep cost volume as include/gsr.h defines it, restated in torch with a dtype switch (`cost_volume`: the yardstick of
tests/test_cost_volume.py in float64 and the source of its bars in float32), the same volume in the form the reference computes it
(`cost_volume_torch_form`: `F.grid_sample` on a (C, D h, w) grid per other view, a product and a sum - what tools/cost_volume_prof.py
times), and the seeded rigs of the tests."""
import math

import torch
import torch.nn.functional as F


def candidates(near, far, num, dtype):
    """(b, v, D) depths: lin formed in float32, the rest in `dtype`."""
    lin = torch.linspace(0.0, 1.0, num, dtype=torch.float32).to(device=near.device, dtype=dtype)
    lo, hi = 1.0 / far.to(dtype), 1.0 / near.to(dtype)
    return 1.0 / (lo[..., None] + lin * (hi - lo)[..., None])


def sample_positions(intrinsics, extrinsics, near, far, num, h, w, i, j, dtype):
    """px, py (b, D, h, w) of row i's pixels in view j, in pixel-index units."""
    K = intrinsics.to(dtype)[:, i].clone()
    K[:, 0] = K[:, 0] * w
    K[:, 1] = K[:, 1] * h
    E = extrinsics.to(dtype)
    P = torch.linalg.inv(E[:, j]) @ E[:, i]
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype, device=K.device), torch.arange(w, dtype=dtype, device=K.device), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(3, -1)                # (3, hw)
    rays = P[:, :3, :3] @ (torch.linalg.inv(K) @ pix)                                 # (b, 3, hw)
    depth = candidates(near, far, num, dtype)[:, i]                                   # (b, D)
    pts = rays[:, :, None, :] * depth[:, None, :, None] + P[:, :3, 3][:, :, None, None]  # (b, 3, D, hw)
    q = torch.einsum("brc,bcdn->brdn", K, pts)
    z = q[:, 2].clamp(min=1e-3)
    return (q[:, 0] / z).reshape(-1, num, h, w), (q[:, 1] / z).reshape(-1, num, h, w)


def bilinear_zero_pad(feat, px, py):
    """feat (b, c, h, w) sampled at px, py (b, D, h, w): (b, c, D, h, w); taps outside the image contribute 0."""
    b, c, h, w = feat.shape
    x0, y0 = torch.floor(px), torch.floor(py)
    flat = feat.reshape(b, c, h * w)
    out = 0
    for dx in (0, 1):
        for dy in (0, 1):
            tx, ty = x0 + dx, y0 + dy
            wgt = (1 - (px - tx).abs()) * (1 - (py - ty).abs())
            inside = (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)
            idx = torch.where(inside, ty * w + tx, torch.zeros_like(tx)).long().reshape(b, 1, -1).expand(b, c, -1)
            tap = torch.gather(flat, 2, idx).reshape(b, c, *px.shape[1:])
            out = out + torch.where(inside, wgt, torch.zeros_like(wgt))[:, None] * tap
    return out


def cost_volume(features, intrinsics, extrinsics, near, far, num, dtype=None):
    """(v b, D, h, w), view-major, in `dtype` (default: the features'); differentiable in `features`."""
    b, v, c, h, w = features.shape
    dtype = dtype or features.dtype
    f = features.to(dtype)
    rows = []
    for i in range(v):
        total = 0
        for k in range(1, v):
            j = (i + k) % v
            with torch.no_grad():
                px, py = sample_positions(intrinsics, extrinsics, near, far, num, h, w, i, j, dtype)
            total = total + (f[:, i, :, None] * bilinear_zero_pad(f[:, j], px, py)).sum(1) / math.sqrt(c)
        rows.append(total / (v - 1))
    return torch.cat(rows, 0)


def cost_volume_torch_form(features, intrinsics, extrinsics, near, far, num):
    """The same volume the way the reference evaluates it, in the features' dtype: per other view the warped features
    (b, c, D, h, w) from `F.grid_sample` on a (D h, w) grid, times the row's features, summed over c."""
    b, v, c, h, w = features.shape
    dtype = features.dtype
    rows = []
    for i in range(v):
        total = 0
        for k in range(1, v):
            j = (i + k) % v
            with torch.no_grad():
                px, py = sample_positions(intrinsics, extrinsics, near, far, num, h, w, i, j, dtype)
                grid = torch.stack([2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1], -1).reshape(b, num * h, w, 2)
            warped = F.grid_sample(features[:, j], grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(b, c, num, h, w)
            total = total + (features[:, i].unsqueeze(2) * warped).sum(1) / c ** 0.5
        rows.append(total / (v - 1))
    return torch.cat(rows, 0)


def rotation(axis_angle):
    """Rodrigues: (..., 3) -> (..., 3, 3), float64."""
    theta = axis_angle.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    k = axis_angle / theta
    Kx = torch.zeros(*axis_angle.shape[:-1], 3, 3, dtype=axis_angle.dtype)
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    t = theta[..., None]
    return torch.eye(3, dtype=axis_angle.dtype) + torch.sin(t) * Kx + (1 - torch.cos(t)) * (Kx @ Kx)


def build_case(seed, b, v, c, h, w, num, spread, kind="random"):
    """Seeded float32 inputs: features ~ N(0, 1); intrinsics near (f, f, 0.5, 0.5), f in 0.8 .. 1.2, per view; camera-to-world poses
    a rotation of up to `spread` radians per axis and a translation of up to `spread` around the origin; near 0.1 .. 0.2, far 50 .. 100;
    a cotangent ~ N(0, 1).  kind "behind": view 1.. turned by 180 degrees about y; "identity": every view the same features and camera."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    features = torch.randn(b, v, c, h, w, generator=g, dtype=torch.float64)
    K = torch.zeros(b, v, 3, 3, dtype=torch.float64)
    K[..., 0, 0], K[..., 1, 1] = 0.8 + 0.4 * u(b, v), 0.8 + 0.4 * u(b, v)
    K[..., 0, 2], K[..., 1, 2] = 0.5 + 0.02 * (u(b, v) - 0.5), 0.5 + 0.02 * (u(b, v) - 0.5)
    K[..., 2, 2] = 1.0
    E = torch.zeros(b, v, 4, 4, dtype=torch.float64)
    E[..., :3, :3] = rotation(spread * (2 * u(b, v, 3) - 1))
    E[..., :3, 3] = spread * (2 * u(b, v, 3) - 1)
    E[..., 3, 3] = 1.0
    near, far = 0.1 + 0.1 * u(b, v), 50.0 + 50.0 * u(b, v)
    if kind == "behind":
        flip = torch.diag(torch.tensor([-1.0, 1.0, -1.0], dtype=torch.float64))
        E[:, 1:, :3, :3] = E[:, 1:, :3, :3] @ flip
    if kind == "identity":
        features = features[:, :1].expand(b, v, c, h, w).contiguous()
        K = K[:, :1].expand(b, v, 3, 3).contiguous()
        E = E[:, :1].expand(b, v, 4, 4).contiguous()
    cot = torch.randn(v * b, num, h, w, generator=g, dtype=torch.float64)
    f32 = lambda t: t.to(torch.float32)
    return {"features": f32(features), "intrinsics": f32(K), "extrinsics": f32(E), "near": f32(near), "far": f32(far), "cotangent": f32(cot),
            "num": num}


def value_and_grad(fn, case, dtype):
    """fn's volume on the case's inputs in `dtype` and dL/dfeatures for the case's cotangent."""
    f = case["features"].to(dtype).clone().requires_grad_(True)
    cost = fn(f, case["intrinsics"].to(dtype), case["extrinsics"].to(dtype), case["near"].to(dtype), case["far"].to(dtype), case["num"])
    (grad,) = torch.autograd.grad(cost, f, case["cotangent"].to(cost.dtype))
    return cost.detach(), grad


def rel_l2(x, ref):
    x, ref = x.double().cpu(), ref.double().cpu()
    den = float(ref.norm())
    return float((x - ref).norm()) / den if den > 0 else float((x - ref).norm())
