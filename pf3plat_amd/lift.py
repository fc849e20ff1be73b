"""The encoder's depth lift on the device (reference src/model/encoder/encoder_costvolume.py:265, 287-307, 506, 525-528 and, for the ray
map, :211-221, 387-392; the definition is stated in include/gsr.h): `lift_depth` turns the mono-depth network's output and the
predicted shift into the refined depth, the per-pixel points `xyz` - what `pose.coarse_poses` and `losses.pose_loss` read - and the
one-hot mono cue that sits next to the cost volume, in one launch each way (gsr_lift_depth / gsr_lift_depth_backward);
`plucker_rays` is the ray map of the pose refinement (gsr_plucker_rays).  There is no CPU fallback."""
from __future__ import annotations

from typing import NamedTuple, Tuple

import torch
from torch import Tensor

from . import _lib
from ._call import f32, launch, ptr, require_device, scratch


class LiftedDepth(NamedTuple):
    depth: Tensor     # ((b v), 1, h, w)
    xyz: Tensor       # (b, v, 3, h, w)
    mono_cue: Tensor  # ((v b), D, h // 4, w // 4), one-hot, no gradient


def _lift_args(depth_raw, shift, near, far, intrinsics, num_candidates):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if near.dim() != 2:
        raise ValueError(f"lift_depth: expected near (b, v), got {tuple(near.shape)}")
    b, v = near.shape
    if v < 1:
        raise ValueError(f"lift_depth: needs at least one view, got {v}")
    if tuple(far.shape) != (b, v):
        raise ValueError(f"lift_depth: expected near, far (b, v) = ({b}, {v}), got {tuple(near.shape)}, {tuple(far.shape)}")
    if depth_raw.dim() != 4 or depth_raw.shape[0] != b * v or depth_raw.shape[1] != 1:
        raise ValueError(f"lift_depth: expected depth_raw ((b v), 1, h, w) = ({b * v}, 1, h, w), got {tuple(depth_raw.shape)}")
    h, w = depth_raw.shape[2:]
    if h < 4 or w < 4:
        raise ValueError(f"lift_depth: needs h >= 4 and w >= 4 (the cue is of (h // 4, w // 4) pixels), got h={h}, w={w}")
    if tuple(shift.shape) != (b * v, 1, h, w):
        raise ValueError(f"lift_depth: expected shift ((b v), 1, h, w) = ({b * v}, 1, {h}, {w}), got {tuple(shift.shape)}")
    if tuple(intrinsics.shape) != (b, v, 3, 3):
        raise ValueError(f"lift_depth: expected intrinsics (b, v, 3, 3) = ({b}, {v}, 3, 3), got {tuple(intrinsics.shape)}")
    d = int(num_candidates)
    if d < 1:
        raise ValueError(f"lift_depth: needs at least one depth candidate, got {num_candidates}")
    limit = 0x7fffffff
    if b * v * 3 * h * w > limit or b * v * d * (h // 4) * (w // 4) > limit:
        raise ValueError("lift_depth: more than 2^31 - 1 elements in the points or the cue")
    require_device("lift", "lift_depth", (depth_raw, shift, near, far, intrinsics))
    return b, v, h, w, d


class _LiftDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_raw, shift, near, far, intrinsics, num_candidates):
        b, v, h, w, d = _lift_args(depth_raw, shift, near, far, intrinsics, num_candidates)
        dev = depth_raw.device
        arrays = (f32(depth_raw), f32(shift), f32(near), f32(far), f32(intrinsics))
        depth = torch.empty((b * v, 1, h, w), dtype=torch.float32, device=dev)  # (all three fully written by the call)
        xyz = torch.empty((b, v, 3, h, w), dtype=torch.float32, device=dev)
        cue = torch.empty((v * b, d, h // 4, w // 4), dtype=torch.float32, device=dev)
        launch("gsr_lift_depth", dev, b, v, h, w, d, *(t.data_ptr() for t in arrays), None, depth.data_ptr(), xyz.data_ptr(), cue.data_ptr())
        ctx.save_for_backward(depth_raw, shift, near, far, intrinsics)
        ctx.sizes = (b, v, h, w)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(cue)
        return depth, xyz, cue

    @staticmethod
    def backward(ctx, g_depth, g_xyz, _g_cue):
        depth_raw, shift, near, far, intrinsics = ctx.saved_tensors
        b, v, h, w = ctx.sizes
        need_raw, need_shift, _, _, need_intr = ctx.needs_input_grad[:5]
        if not (need_raw or need_shift or need_intr) or (g_depth is None and g_xyz is None):
            return None, None, None, None, None, None
        dev = depth_raw.device
        arrays = (f32(depth_raw), f32(shift), f32(near), f32(far), f32(intrinsics))
        ups = [None if g is None else f32(g) for g in (g_depth, g_xyz)]
        d_raw = torch.empty((b * v, 1, h, w), dtype=torch.float32, device=dev) if need_raw else None  # (fully written by the call)
        d_shift = torch.empty((b * v, 1, h, w), dtype=torch.float32, device=dev) if need_shift else None
        d_intr = torch.empty((b, v, 3, 3), dtype=torch.float32, device=dev) if need_intr else None
        work = scratch(_lib.load().gsr_lift_scratch_bytes(b, v, h, w), torch.float64, dev) if need_intr else None
        launch("gsr_lift_depth_backward", dev, b, v, h, w, *(t.data_ptr() for t in arrays), ptr(ups[0]), ptr(ups[1]), ptr(d_raw), ptr(d_shift),
               ptr(d_intr), ptr(work))
        return (d_raw.to(depth_raw.dtype) if need_raw else None, d_shift.to(shift.dtype) if need_shift else None, None, None,
                d_intr.to(intrinsics.dtype) if need_intr else None, None)


def lift_depth(depth_raw: Tensor, shift: Tensor, near: Tensor, far: Tensor, intrinsics: Tensor, num_candidates: int = 128) -> LiftedDepth:
    """depth_raw, shift ((b v), 1, h, w), near, far (b, v), normalised intrinsics (b, v, 3, 3) -> LiftedDepth as include/gsr.h
    defines it: depth = clamp(clamp(depth_raw, near, far) + shift, near, far), bit-equal to the float32 torch form; xyz (b, v, 3, h, w)
    = K^-1 (pixel centre, 1) depth; mono_cue ((v b), D, h // 4, w // 4), view-major, the one-hot of argmin_d |down - hyp_d| with `down` the
    bilinear quarter-resolution depth.  Two quirks of the reference are kept: the hypotheses are INVERSE depths compared with a depth,
    and they come from near[0, 0], far[0, 0] for the whole batch.  Differentiable in depth_raw and shift, and in intrinsics when that
    tensor requires grad (a second, small launch; bit-reproducible); near, far and the cue get no gradient.  One launch each way, no
    host synchronisation.  v = 1 is allowed.  Inputs that are not float32 or not contiguous are converted."""
    return LiftedDepth(*_LiftDepth.apply(depth_raw, shift, near, far, intrinsics, int(num_candidates)))


def plucker_rays(c2w: Tensor, intrinsics: Tensor, shape: Tuple[int, int]) -> Tensor:
    """c2w (b, v, 4, 4) camera-to-world, normalised intrinsics (b, v, 3, 3), shape = (H, W) -> ((b v), 6, H, W), float32: the world-space
    unit ray direction of every pixel centre (normalised in camera space, then rotated) and cross(camera position, direction), as the
    reference's get_world_rays + plucker_embedding.  One launch; no gradient."""
    if c2w.dim() != 4 or tuple(c2w.shape[2:]) != (4, 4):
        raise ValueError(f"plucker_rays: expected c2w (b, v, 4, 4), got {tuple(c2w.shape)}")
    b, v = c2w.shape[:2]
    if v < 1:
        raise ValueError(f"plucker_rays: needs at least one view, got {v}")
    if tuple(intrinsics.shape) != (b, v, 3, 3):
        raise ValueError(f"plucker_rays: expected intrinsics (b, v, 3, 3) = ({b}, {v}, 3, 3), got {tuple(intrinsics.shape)}")
    if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
        raise ValueError(f"plucker_rays: expected shape (H, W) with H, W >= 1, got {tuple(shape)}")
    H, W = int(shape[0]), int(shape[1])
    if b * v * 6 * H * W > 0x7fffffff:
        raise ValueError("plucker_rays: more than 2^31 - 1 elements in the ray map")
    require_device("lift", "plucker_rays", (c2w, intrinsics))
    arrays = (f32(c2w), f32(intrinsics))
    out = torch.empty((b * v, 6, H, W), dtype=torch.float32, device=c2w.device)
    launch("gsr_plucker_rays", c2w.device, b, v, H, W, *(t.data_ptr() for t in arrays), out.data_ptr())
    return out
