"""The encoder's plane-sweep cost volume on the device (reference src/model/encoder/costvolume/depth_predictor_multiview.py:28-141,
321-343; the definition is stated in include/gsr.h): `plane_sweep_cost_volume` replaces `prepare_feat_proj_data_lists`, the
`warp_with_pose_depth_candidates` calls and the correlation of `DepthPredictorMultiView.forward` with one launch chain each way
(gsr_cost_volume / gsr_cost_volume_backward); the warped features (v b, c, D, h, w) are never formed.  There is no CPU fallback."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib
from ._call import f32, launch, require_device, scratch


def _cost_volume_args(features, intrinsics, extrinsics, near, far, num_depth_candidates):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if features.dim() != 5:
        raise ValueError(f"plane_sweep_cost_volume: expected features (b, v, c, h, w), got {tuple(features.shape)}")
    b, v, c, h, w = features.shape
    if v < 2:
        raise ValueError(f"plane_sweep_cost_volume: needs at least two views, got {v}")
    if c < 1 or h < 2 or w < 2:
        raise ValueError(f"plane_sweep_cost_volume: needs c >= 1, h >= 2 and w >= 2 (the warp divides by w - 1 and h - 1), got c={c}, h={h}, w={w}")
    if tuple(intrinsics.shape) != (b, v, 3, 3):
        raise ValueError(f"plane_sweep_cost_volume: expected intrinsics (b, v, 3, 3) = ({b}, {v}, 3, 3), got {tuple(intrinsics.shape)}")
    if tuple(extrinsics.shape) != (b, v, 4, 4):
        raise ValueError(f"plane_sweep_cost_volume: expected extrinsics (b, v, 4, 4) = ({b}, {v}, 4, 4), got {tuple(extrinsics.shape)}")
    if tuple(near.shape) != (b, v) or tuple(far.shape) != (b, v):
        raise ValueError(f"plane_sweep_cost_volume: expected near, far (b, v) = ({b}, {v}), got {tuple(near.shape)}, {tuple(far.shape)}")
    d = int(num_depth_candidates)
    if d < 1:
        raise ValueError(f"plane_sweep_cost_volume: needs at least one depth candidate, got {num_depth_candidates}")
    limit = 0x7fffffff
    if b * v * h * w * ((c + 3) // 4 * 4) > limit or b * v * d * h * w > limit:
        raise ValueError("plane_sweep_cost_volume: more than 2^31 - 1 elements in the features or the volume")
    require_device("cost_volume", "plane_sweep_cost_volume", (features, intrinsics, extrinsics, near, far))
    return b, v, c, h, w, d


def _scratch(sizes, backward: bool, dev) -> Tensor:
    b, v, c, h, w, _ = sizes
    return scratch(_lib.load().gsr_cost_volume_scratch_bytes(b, v, c, h, w, int(backward)), torch.float32, dev)


class _CostVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, intrinsics, extrinsics, near, far, num_depth_candidates):
        sizes = _cost_volume_args(features, intrinsics, extrinsics, near, far, num_depth_candidates)
        b, v, c, h, w, d = sizes
        dev = features.device
        arrays = (f32(features), f32(intrinsics), f32(extrinsics), f32(near), f32(far))
        cost = torch.empty((v * b, d, h, w), dtype=torch.float32, device=dev)
        work = _scratch(sizes, False, dev)  # (the backward allocates its own: nothing but the inputs outlives this call)
        launch("gsr_cost_volume", dev, *sizes, *(t.data_ptr() for t in arrays), cost.data_ptr(), work.data_ptr())
        ctx.save_for_backward(features, intrinsics, extrinsics, near, far)
        ctx.sizes = sizes
        return cost

    @staticmethod
    def backward(ctx, g_cost):
        features, intrinsics, extrinsics, near, far = ctx.saved_tensors
        sizes = ctx.sizes
        b, v, c, h, w, _ = sizes
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        dev = features.device
        arrays = (f32(features), f32(intrinsics), f32(extrinsics), f32(near), f32(far))
        d_features = torch.empty((b, v, c, h, w), dtype=torch.float32, device=dev)  # (fully written by the call)
        work = _scratch(sizes, True, dev)
        up = f32(g_cost)
        launch("gsr_cost_volume_backward", dev, *sizes, *(t.data_ptr() for t in arrays), up.data_ptr(), d_features.data_ptr(), work.data_ptr())
        return d_features.to(features.dtype), None, None, None, None, None


def plane_sweep_cost_volume(features: Tensor, intrinsics: Tensor, extrinsics: Tensor, near: Tensor, far: Tensor,
                            num_depth_candidates: int) -> Tensor:
    """features (b, v, c, h, w), normalised intrinsics (b, v, 3, 3), camera-to-world extrinsics (b, v, 4, 4), near, far (b, v) ->
    the cost volume (v b, D, h, w), float32, view-major (row i b + s is view i of scene s) as include/gsr.h defines it: the mean over
    the other views of the correlation of a pixel's feature with the other view's features warped to D inverse-depth candidates.
    Differentiable in `features` only (the reference builds its sampling grid under no_grad); the gradient's last bits can differ from
    run to run (float atomics), the value's do not.  Two launches forward; a zero-fill and three launches backward, with workspace of
    twice the features that lives for that call alone; a forward allocates one copy of the features and no gradient workspace.
    Inputs that are not float32 or not contiguous are converted."""
    return _CostVolume.apply(features, intrinsics, extrinsics, near, far, int(num_depth_candidates))


def depth_candidates(near: Tensor, far: Tensor, num_depth_candidates: int) -> Tensor:
    """The (v b, D) inverse-depth candidates of the volume's rows, 1 / far + linspace(0, 1, D) (1 / near - 1 / far) in the bounds' dtype,
    view-major: what the reference's caller reads right after the volume (`disp_candi_curr`, depth_predictor_multiview.py:132-139)."""
    if near.dim() != 2 or near.shape != far.shape:
        raise ValueError(f"depth_candidates: expected near, far (b, v), got {tuple(near.shape)}, {tuple(far.shape)}")
    if int(num_depth_candidates) < 1:
        raise ValueError(f"depth_candidates: needs at least one depth candidate, got {num_depth_candidates}")
    lo = (1.0 / far.detach()).t().reshape(-1, 1)
    hi = (1.0 / near.detach()).t().reshape(-1, 1)
    lin = torch.linspace(0.0, 1.0, int(num_depth_candidates), dtype=torch.float32, device=near.device).to(lo.dtype)
    return lo + lin.unsqueeze(0) * (hi - lo)
