"""The pose loss (`Losspose`, reference src/loss/loss_pose.py:28-129) as include/gsr.h defines it, restated in torch: `pose_loss`,
vectorised over all matches of a call, with a dtype switch (float64: what the HIP kernels are measured against; float32: what the
same arithmetic loses in the kernels' number format - the tests' bars are multiples of the difference); `pose_loss_loop`, the
same loss in the reference's form (whole-grid projections per pair, then a Python loop over the lists with a handful of small
ops each), which tools/pose_loss_prof.py times next to the kernels; and `build_scene`, the seeded inputs of the tests.  The pixel
centres are float32 in both dtypes, as `sample_image_grid` makes them."""
from __future__ import annotations

from dataclasses import dataclass

import torch

DELTA = 0.01  # the Huber threshold of the 2D term
EPS = 1e-6    # from_homogeneous's epsilon


def pairs_of(v):
    return [(a, c) for a in range(v) for c in range(a + 1, v)]


@dataclass
class Scene:
    xyz: torch.Tensor         # (b, v, 3, h, w) float32
    depth: torch.Tensor       # (b v, 1, h, w) float32
    poses: torch.Tensor       # (b, v, 4, 4) float32, bottom rows (0, 0, 0, 1)
    intrinsics: torch.Tensor  # (b, v, 3, 3) float32
    corr: dict                # {(i, j): [(id_i, id_j, score) per scene]}: the reference's `corr[0]`
    conf: dict                # {(i, j): (b,) tensor}: the reference's `corr[2]`


def _centres(ids, h, w):
    """c(id) = ((id % w + 0.5) / w, (id // w + 0.5) / h), in float32."""
    x = ((ids % w).to(torch.float32) + 0.5) / w
    y = ((ids // w).to(torch.float32) + 0.5) / h
    return torch.stack([x, y], -1)


def _affine(poses):
    """(…, 4, 4) -> the same with the bottom row replaced by the constant (0, 0, 0, 1): only the top rows are read."""
    bottom = torch.zeros_like(poses[..., 3:, :])
    bottom[..., 0, 3] = 1
    return torch.cat([poses[..., :3, :], bottom], -2)


def _affine_inverse(p):
    rinv = torch.linalg.inv(p[..., :3, :3])
    top = torch.cat([rinv, -(rinv @ p[..., :3, 3:])], -1)
    return torch.cat([top, p[..., 3:, :]], -2)


def _huber(r):
    return torch.where(r <= DELTA, 0.5 * r * r, DELTA * (r - 0.5 * DELTA)) / DELTA


def residuals(scene_or_tensors, dtype=torch.float64):
    """-> (r3, r2, list index) of every match of the call, concatenated pair-major then scene."""
    xyz, depth, poses, intr, corr = scene_or_tensors
    b, v, _, h, w = xyz.shape
    xyz, poses, intr = xyz.to(dtype), _affine(poses.to(dtype)), intr.to(dtype)
    depth = depth.to(dtype).reshape(b, v, h * w)
    flat = xyz.reshape(b, v, 3, h * w)
    r3, r2, lid = [], [], []
    for p, (i, j) in enumerate(pairs_of(v)):
        rt = poses[:, j] if i == 0 else poses[:, j] @ _affine_inverse(poses[:, i])
        kinv = torch.linalg.inv(intr[:, i])
        for s in range(b):
            a, c, _ = corr[(i, j)][s]
            R, t = rt[s, :3, :3], rt[s, :3, 3]
            r3.append((flat[s, i][:, a].T @ R.T + t - flat[s, j][:, c].T).norm(dim=-1))
            ca = torch.cat([_centres(a, h, w).to(dtype), torch.ones((len(a), 1), dtype=dtype)], -1)
            P = (ca @ kinv[s].T) * depth[s, i][a][:, None]
            Q = (P @ R.T + t) / (1 + EPS)
            u = Q @ intr[s, j].T
            q = u[:, :2] / (u[:, 2:] + EPS)
            r2.append((q - _centres(c, h, w).to(dtype)).norm(dim=-1))
            lid.append(torch.full((len(a),), p * b + s))
    return torch.cat(r3), torch.cat(r2), torch.cat(lid)


def pose_loss(xyz, depth, poses, intrinsics, corr, conf, weight_2d, weight_3d, dtype=torch.float64, per_list=False):
    """-> (loss, mean L3, mean L2); differentiable in xyz, depth and (the top three rows of) poses.  per_list: a fourth entry,
    (l3, l2, sum |score|) of every list in the kernels' list order (pair-major, then scene) - l3 with its confidence and its
    normalisation, the sum of the scores as it is (not clamped)."""
    b, v = xyz.shape[:2]
    lists = b * len(pairs_of(v))
    r3, r2, lid = residuals((xyz, depth, poses, intrinsics, corr), dtype)
    order = [(p, s) for p in pairs_of(v) for s in range(b)]
    wgt = torch.cat([corr[p][s][2] for p, s in order]).to(dtype)
    cf = torch.stack([torch.as_tensor(conf[p][s]) for p, s in order]).to(dtype).reshape(lists)
    zero = torch.zeros(lists, dtype=dtype)
    sw = zero.index_add(0, lid, wgt.abs())
    l3 = cf * zero.index_add(0, lid, wgt * r3) / sw.clamp_min(1e-12)
    l2 = zero.index_add(0, lid, _huber(r2))
    m3, m2 = l3.mean(), l2.mean()
    loss = weight_3d * m3 + weight_2d * m2
    return (loss, m3, m2, (l3, l2, sw)) if per_list else (loss, m3, m2)


def pose_loss_loop(xyz, depth, poses, intrinsics, corr, conf, weight_2d, weight_3d):
    """The same loss the way the reference evaluates it, in the inputs' dtype and on their device: per pair the WHOLE grid of every
    scene is projected into the other view, then every (scene, pair) list gathers from it and forms its two terms with a few small
    ops.  This is the form the kernels replace; it is here to be timed, and is checked against `pose_loss` on the CPU."""
    b, v, _, h, w = xyz.shape
    dev = xyz.device
    ids = torch.arange(h * w, device=dev)
    grid = _centres(ids, h, w).to(xyz.dtype)
    grid1 = torch.cat([grid, torch.ones_like(grid[:, :1])], -1)
    depth = depth.reshape(b, v, h * w)
    poses = _affine(poses)
    rts, proj = {}, {}
    for i, j in pairs_of(v):
        rt = poses[:, j] if i == 0 else poses[:, j] @ _affine_inverse(poses[:, i])
        P = (grid1 @ torch.linalg.inv(intrinsics[:, i]).transpose(-1, -2)) * depth[:, i, :, None]
        Q = (P @ rt[:, :3, :3].transpose(-1, -2) + rt[:, None, :3, 3]) / (1 + EPS)
        u = Q @ intrinsics[:, j].transpose(-1, -2)
        rts[i, j], proj[i, j] = rt, u[..., :2] / (u[..., 2:] + EPS)
    l3, l2 = [], []
    for s in range(b):
        for i, j in pairs_of(v):
            a, c, score = corr[(i, j)][s]
            rt = rts[i, j][s]
            xi = xyz[s, i].flatten(-2, -1).T[a]
            xj = xyz[s, j].flatten(-2, -1).T[c]
            r3 = (xi @ rt[:3, :3].T + rt[:3, 3] - xj).norm(dim=-1)
            l3.append((torch.nn.functional.normalize(score, p=1, dim=-1) * r3).sum() * conf[(i, j)][s])
            l2.append(_huber((proj[i, j][s][a] - grid[c]).norm(dim=-1)).sum())
    m3, m2 = torch.stack(l3).mean(), torch.stack(l2).mean()
    return weight_3d * m3 + weight_2d * m2, m3, m2


def _rotation(g, angle):
    axis = torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
    a = angle * (2 * torch.rand((), generator=g, dtype=torch.float64) - 1)
    k = torch.zeros(3, 3, dtype=torch.float64)
    k[0, 1], k[0, 2], k[1, 0], k[1, 2], k[2, 0], k[2, 1] = -axis[2], axis[1], axis[2], -axis[0], -axis[1], axis[0]
    return torch.eye(3, dtype=torch.float64) + torch.sin(a) * k + (1 - torch.cos(a)) * (k @ k)


def build_scene(seed, b, v, h, w, lengths, kinds, zero_weight_lists=(), repeat_lists=(), exact=False, signed_lists=(), corner_lists=()) -> Scene:
    """Seeded inputs.  lengths: one per list, pair-major then scene.  kinds: one per scene -
      "near":   every pose within 1e-3 of the identity, one K for the scene's views, id_j = id_i and x_j = x_i + 1e-2 noise: the
                reprojection lands within ~1e-3 of the pixel it left, the QUADRATIC side of the Huber threshold 0.01;
      "random": general poses (view 0 included: the i == 0 shortcut must not read it), a K per view, unrelated random ids: the
                reprojection misses by a good part of the image, the LINEAR side.
    zero_weight_lists: lists whose scores are all 0.  repeat_lists: lists whose every entry names one pixel pair.  signed_lists:
    lists whose scores carry a random sign each, |score| in [0.05, 1] as everywhere (the L1 norm is of |score|).  corner_lists: lists
    whose first two matches name pixel 0 and pixel h * w - 1 in the first view - and the same two in the second view of a "near" scene,
    crossed (h * w - 1, then 0) in that of a "random" one.  Neither option draws a number in a list it does not name.  exact: poses
    that are translations by multiples of 1 / 8, one K, and ONE point (multiples of 1 / 8 too) on every pixel of a scene, moved by
    each view's translation - the 3D residual of any two ids is exactly 0 in either precision (the norm's gradient there is taken
    as 0), while the ids, and with them the 2D term and the depth's gradient, stay those of the scene's kind."""
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    rand = lambda *s: torch.rand(s, generator=g, dtype=f64)
    randn = lambda *s: torch.randn(s, generator=g, dtype=f64)
    poses = torch.eye(4, dtype=f64).repeat(b, v, 1, 1)
    intr = torch.zeros(b, v, 3, 3, dtype=f64)
    xyz = torch.zeros(b, v, 3, h, w, dtype=f64)
    for s in range(b):
        base = torch.cat([randn(2, h, w), 2 + 2 * rand(1, h, w)])
        k0 = torch.tensor([[0.8 + 0.3 * rand().item(), 0, 0.5], [0, 0.9 + 0.3 * rand().item(), 0.5], [0, 0, 1]], dtype=f64)
        for u in range(v):
            if exact:  # multiples of 1 / 8: x + t is exact in float32 and float64 alike
                point = torch.cat([torch.randint(-8, 9, (2,), generator=g), torch.randint(16, 32, (1,), generator=g)]).to(f64) / 8
                point = point if u == 0 else xyz[s, 0, :, 0, 0]
                poses[s, u, :3, 3] = 0 if u == 0 else torch.randint(-4, 5, (3,), generator=g).to(f64) / 8
                intr[s, u] = k0
                xyz[s, u] = (point + poses[s, u, :3, 3])[:, None, None].expand(3, h, w)
            elif kinds[s] == "near":
                intr[s, u] = k0
                xyz[s, u] = base + 1e-2 * randn(3, h, w)
                poses[s, u, :3] += 1e-3 * randn(3, 4)
            else:
                intr[s, u] = k0 + torch.tensor([[0.1, 0.02, 0.03], [0, 0.1, 0.03], [0, 0, 0]], dtype=f64) * randn(3, 3)
                xyz[s, u] = torch.cat([randn(2, h, w), 2 + 2 * rand(1, h, w)])
                # a general 3 x 3 (a rotation, sheared a little: the inverse is no transpose) and a translation
                poses[s, u, :3, :3] = _rotation(g, 0.6) @ (torch.eye(3, dtype=f64) + 0.05 * randn(3, 3))
                poses[s, u, :3, 3] = 0.3 * randn(3)
    depth = 1 + 3 * rand(b * v, 1, h, w)
    corr, conf, at = {}, {}, 0
    for p in pairs_of(v):
        corr[p], conf[p] = [], (0.2 + 0.8 * rand(b)).to(torch.float32)
        for s in range(b):
            n = lengths[at]
            a = torch.randint(0, h * w, (n,), generator=g)
            if at in corner_lists:
                a[0], a[1] = 0, h * w - 1
            c = a.clone() if kinds[s] == "near" else torch.randint(0, h * w, (n,), generator=g)
            if at in repeat_lists:
                a, c = a[:1].repeat(n), c[:1].repeat(n)
            if at in corner_lists and kinds[s] != "near":
                c[0], c[1] = h * w - 1, 0
            score = torch.zeros(n) if at in zero_weight_lists else (0.05 + 0.95 * rand(n)).to(torch.float32)
            if at in signed_lists:
                score = score * (2 * torch.randint(0, 2, (n,), generator=g) - 1).to(torch.float32)
            corr[p].append((a, c, score))
            at += 1
    assert at == len(lengths) == b * len(pairs_of(v))
    f32 = torch.float32
    return Scene(xyz.to(f32), depth.to(f32), poses.to(f32), intr.to(f32), corr, conf)
