"""The depth lift and the Pluecker ray map as include/gsr.h defines them, restated in torch with a dtype switch: the yardstick of
tests/test_lift.py in float64 and the source of its bars in float32 (what tools/lift_time.py times as the eager torch form), and the
seeded cases of the tests."""
import torch
import torch.nn.functional as F

from tests.cost_volume_ref import rotation  # noqa: F401  (Rodrigues, float64; the tests' planted scenes use it too)


def refined_depth(depth_raw, shift, near, far):
    """((b v), 1, h, w): both clamps with the view's own bounds; differentiable in depth_raw and shift."""
    lo, hi = near.reshape(-1, 1, 1, 1).to(depth_raw.dtype), far.reshape(-1, 1, 1, 1).to(depth_raw.dtype)
    return (depth_raw.clamp(lo, hi) + shift).clamp(lo, hi)


def pixel_centres(h, w, dtype, device="cpu"):
    """(3, h w): ((x + .5) / w, (y + .5) / h, 1) of every pixel, row-major."""
    ys, xs = torch.meshgrid((torch.arange(h, dtype=dtype, device=device) + 0.5) / h, (torch.arange(w, dtype=dtype, device=device) + 0.5) / w,
                            indexing="ij")
    return torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(3, -1)


def points(depth, intrinsics):
    """(b, v, 3, h, w) = K^-1 (pixel centre, 1) depth; differentiable in depth and intrinsics."""
    b, v = intrinsics.shape[:2]
    h, w = depth.shape[-2:]
    rays = torch.linalg.inv(intrinsics) @ pixel_centres(h, w, depth.dtype, depth.device)  # (b, v, 3, hw)
    return rays.reshape(b, v, 3, h, w) * depth.reshape(b, v, 1, h, w)


def hypotheses(near, far, num, dtype):
    """(D): 1 / far[0, 0] + lin (1 / near[0, 0] - 1 / far[0, 0]); lin is float32's linspace.  INVERSE depths, of scene 0, view 0."""
    lin = torch.linspace(0.0, 1.0, num, dtype=torch.float32).to(device=near.device, dtype=dtype)
    lo, hi = 1.0 / far[0, 0].to(dtype), 1.0 / near[0, 0].to(dtype)
    return lo + lin * (hi - lo)


def cue_channels(depth, near, far, num, hyp=None):
    """The cue's channel per quarter pixel, (v b, h // 4, w // 4) int64, view-major rows, and the gap between the two smallest
    |down - hyp| in units of the hypothesis spacing (inf for D = 1): a pixel is `decided` when its gap exceeds 1e-3."""
    b, v = near.shape
    h, w = depth.shape[-2:]
    with torch.no_grad():
        down = F.interpolate(depth.detach(), (h // 4, w // 4), mode="bilinear")                   # ((b v), 1, hq, wq)
        hyp = hypotheses(near, far, num, depth.dtype) if hyp is None else hyp
        diff = (down - hyp.view(1, -1, 1, 1)).abs()                                               # ((b v), D, hq, wq)
        channel = diff.argmin(dim=1)
        if num > 1:
            two = diff.double().topk(2, dim=1, largest=False).values
            gap = (two[:, 1] - two[:, 0]) / float((hyp[-1] - hyp[0]).abs().double() / (num - 1))
        else:
            gap = torch.full(channel.shape, float("inf"), dtype=torch.float64)
    to_view_major = lambda t: t.reshape(b, v, *t.shape[1:]).transpose(0, 1).reshape(v * b, *t.shape[1:])
    return to_view_major(channel), to_view_major(gap)


def mono_cue(depth, near, far, num):
    """The cue itself, ((v b), D, h // 4, w // 4) in the depth's dtype, as eager torch ops on the depth's device (no host read of the
    bounds): the resize, |down - hyp| over the whole volume, the argmin and a scatter of ones into zeros."""
    b, v = near.shape
    h, w = depth.shape[-2:]
    with torch.no_grad():
        down = F.interpolate(depth.detach(), (h // 4, w // 4), mode="bilinear")
        diff = (down - hypotheses(near, far, num, depth.dtype).view(1, -1, 1, 1)).abs()
        cue = torch.zeros_like(diff).scatter_(1, diff.argmin(dim=1, keepdim=True), 1.0)
    return cue.reshape(b, v, *cue.shape[1:]).transpose(0, 1).reshape(v * b, *cue.shape[1:])


def lift(depth_raw, shift, near, far, intrinsics):
    depth = refined_depth(depth_raw, shift, near, far)
    return depth, points(depth, intrinsics)


def plucker(c2w, intrinsics, H, W):
    """((b v), 6, H, W): unit directions (normalised in camera space, then rotated into the world), cross(camera position, direction)."""
    b, v = intrinsics.shape[:2]
    rays = torch.linalg.inv(intrinsics) @ pixel_centres(H, W, intrinsics.dtype, intrinsics.device)  # (b, v, 3, HW)
    rays = rays / rays.norm(dim=2, keepdim=True)
    world = c2w[:, :, :3, :3] @ rays
    origin = c2w[:, :, :3, 3:].expand_as(world)
    moment = torch.cross(origin, world, dim=2)
    return torch.cat([world, moment], 2).reshape(b * v, 6, H, W)


def build_case(seed, b, v, h, w, num, kind="plain"):
    """Seeded float32 inputs.  depth_raw uniform in [.3, 2.3], shift ~ .3 N(0, 1), near = .5, far = 2 (about a quarter of the pixels end
    on a bound); intrinsics near (f, f, .5, .5), f in .8 .. 1.2 per view; camera-to-world poses a rotation of up to .5 rad per axis and a
    translation of up to 1; cotangents ~ N(0, 1) for depth and xyz.
    kind "per_view": near[0, 0] = .5, far[0, 0] = 2 and every other view near in .55 .. .65, far in 1.7 .. 1.9;
    kind "full_k": skew and a general third row in the intrinsics."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    n = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    depth_raw = 0.3 + 2.0 * u(b * v, 1, h, w)
    shift = 0.3 * n(b * v, 1, h, w)
    K = torch.zeros(b, v, 3, 3, dtype=torch.float64)
    K[..., 0, 0], K[..., 1, 1] = 0.8 + 0.4 * u(b, v), 0.8 + 0.4 * u(b, v)
    K[..., 0, 2], K[..., 1, 2] = 0.5 + 0.02 * (u(b, v) - 0.5), 0.5 + 0.02 * (u(b, v) - 0.5)
    K[..., 2, 2] = 1.0
    E = torch.zeros(b, v, 4, 4, dtype=torch.float64)
    E[..., :3, :3] = rotation(0.5 * (2 * u(b, v, 3) - 1))
    E[..., :3, 3] = 2 * u(b, v, 3) - 1
    E[..., 3, 3] = 1.0
    near, far = torch.full((b, v), 0.5, dtype=torch.float64), torch.full((b, v), 2.0, dtype=torch.float64)
    g_depth, g_xyz = n(b * v, 1, h, w), n(b, v, 3, h, w)
    if kind == "per_view":
        near, far = 0.55 + 0.1 * u(b, v), 1.7 + 0.2 * u(b, v)
        near[0, 0], far[0, 0] = 0.5, 2.0
    if kind == "full_k":
        K[..., 0, 1] = 0.1 * (u(b, v) - 0.5)
        K[..., 1, 0] = 0.05 * (u(b, v) - 0.5)
        K[..., 2, 0], K[..., 2, 1] = 0.1 * (u(b, v) - 0.5), 0.1 * (u(b, v) - 0.5)
        K[..., 2, 2] = 0.9 + 0.2 * u(b, v)
    f32 = lambda t: t.to(torch.float32)
    return {"depth_raw": f32(depth_raw), "shift": f32(shift), "near": f32(near), "far": f32(far), "intrinsics": f32(K), "c2w": f32(E),
            "g_depth": f32(g_depth), "g_xyz": f32(g_xyz), "num": num}


def evaluate(case, dtype):
    """Everything the tests compare, on the case's inputs in `dtype`: depth, xyz, the cue's channels and gaps, the gradients of
    sum(depth g_depth) + sum(xyz g_xyz) for depth_raw, shift and intrinsics."""
    raw = case["depth_raw"].to(dtype).clone().requires_grad_(True)
    shift = case["shift"].to(dtype).clone().requires_grad_(True)
    K = case["intrinsics"].to(dtype).clone().requires_grad_(True)
    near, far = case["near"].to(dtype), case["far"].to(dtype)
    depth, xyz = lift(raw, shift, near, far, K)
    d_raw, d_shift, d_K = torch.autograd.grad([depth, xyz], [raw, shift, K], [case["g_depth"].to(dtype), case["g_xyz"].to(dtype)])
    channel, gap = cue_channels(depth, near, far, case["num"])
    return {"depth": depth.detach(), "xyz": xyz.detach(), "channel": channel, "gap": gap, "d_depth_raw": d_raw, "d_shift": d_shift,
            "d_intrinsics": d_K}


def rel_l2(x, ref):
    x, ref = x.double().cpu(), ref.double().cpu()
    den = float(ref.norm())
    return float((x - ref).norm()) / den if den > 0 else float((x - ref).norm())
