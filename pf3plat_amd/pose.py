"""The encoder's coarse camera poses on the device (reference src/model/encoder/encoder_costvolume.py:323-381 and
src/flow_util.py:623-743; the definition is stated in include/gsr.h): `pnp_ransac` replaces the loop of `cv2.solvePnPRansac` calls
over (pair, scene) - and its copies to the host and back - with two launches (gsr_pnp_ransac), `synchronize_cameras` replaces
`camera_synchronization` with one (gsr_camera_sync), and `coarse_poses` is the chain: three launches, no host synchronisation, no
gradient (the reference's poses come back from numpy).  `refine_poses` is what follows the pose transformer (:447-450, 460-473 and
the `.inverse()` calls of :492, :530 and model_wrapper.py:150): the 6D + translation encoding, the head's residual, Gram-Schmidt,
c2w and w2c in one launch each way (gsr_pose_refine / gsr_pose_refine_backward), differentiable in the residual and its gain;
`pose_encoding` is the encoding alone; `pose_errors` the per-step diagnostics of model_wrapper.py:182-190 (gsr_pose_errors).
There is no CPU fallback."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib
from ._call import f32, launch, ptr, require_device, scratch
from .losses import PackedCorrespondences, pack_correspondences

MIN_MATCHES = 4  # a P3P solve on three matches and one to choose its root (gsr_pnp_min_matches)
MAX_VIEWS = 8
STATUS_OK, STATUS_TOO_FEW_MATCHES, STATUS_NO_CONSENSUS, STATUS_NOT_FINITE = 0, 1, 2, 3


@dataclass
class CoarsePoses:
    pairwise: Tensor    # (b, P, 4, 4): the reference's pw_relpose_list, pairs in the pack's order
    absolute: Tensor    # (b, v, 4, 4): the reference's sync_abspose
    confidence: Tensor  # (P b,) in the list order of the pack: what the synchronisation weighs the pairs with
    inliers: Tensor     # (P b,) int32
    status: Tensor      # (P b,) int32: STATUS_*
    mask: Optional[Tensor] = None  # (M,) uint8, on request


def pack_matches(corr) -> PackedCorrespondences:
    """`pack_correspondences` without confidences: the reference's {(i, j): [(id_i, id_j, score) per scene]} as the kernels read it,
    with zeros where the confidences go.  `coarse_poses` returns the confidences; `dataclasses.replace(packed, conf=...)` puts them
    into the pack for the pose loss."""
    pairs = sorted(corr.keys())
    if not pairs:
        raise ValueError("pack_matches: no pairs")
    scores = corr[pairs[0]][0][2] if len(corr[pairs[0]]) else None
    dev = scores.device if scores is not None else None
    conf = {p: torch.zeros(len(corr[p]), dtype=torch.float32, device=dev) for p in pairs}
    return pack_correspondences(corr, conf)


def _pnp_args(xyz, intrinsics_px, packed, points_2d, hypotheses, reprojection_error, confidence_min):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if xyz.dim() != 5 or xyz.shape[2] != 3:
        raise ValueError(f"pnp_ransac: expected xyz (b, v, 3, h, w), got {tuple(xyz.shape)}")
    b, v, _, h, w = xyz.shape
    if v < 2 or v > MAX_VIEWS:
        raise ValueError(f"pnp_ransac: needs 2 to {MAX_VIEWS} views, got {v}")
    if tuple(intrinsics_px.shape) != (b, v, 3, 3):
        raise ValueError(f"pnp_ransac: expected intrinsics_px (b, v, 3, 3) = ({b}, {v}, 3, 3), got {tuple(intrinsics_px.shape)}")
    if packed.num_scenes != b or packed.num_pairs != v * (v - 1) // 2 or len(packed.offsets) != b * packed.num_pairs + 1:
        raise ValueError(f"pnp_ransac: the matches are packed for {packed.num_scenes} scenes and {packed.num_pairs} pairs, "
                         f"the points are of {b} scenes and {v} views ({v * (v - 1) // 2} pairs)")
    total = packed.offsets[-1]
    if points_2d is not None and tuple(points_2d.shape) != (total, 2):
        raise ValueError(f"pnp_ransac: expected points_2d (M, 2) = ({total}, 2), got {tuple(points_2d.shape)}")
    if int(hypotheses) < 1 or int(hypotheses) > 1 << 24:
        raise ValueError(f"pnp_ransac: needs 1 to 2^24 hypotheses, got {hypotheses}")
    if not float(reprojection_error) > 0.0:
        raise ValueError(f"pnp_ransac: needs a positive reprojection_error, got {reprojection_error}")
    if not float(confidence_min) < 1.0:
        raise ValueError(f"pnp_ransac: needs confidence_min < 1, got {confidence_min}")
    if h * w > 0x7fffffff:
        raise ValueError("pnp_ransac: more than 2^31 - 1 pixels in a view")
    tensors = [xyz, intrinsics_px, packed.ids_i, packed.ids_j, packed.weights, packed.offsets_device]
    if points_2d is not None:
        tensors.append(points_2d)
    require_device("pose", "pnp_ransac", tensors)
    return b, v, h, w


def _pnp(xyz, intrinsics_px, packed, points_2d, hypotheses, reprojection_error, confidence_min, seed, return_mask):
    b, v, h, w = _pnp_args(xyz, intrinsics_px, packed, points_2d, hypotheses, reprojection_error, confidence_min)
    dev = xyz.device
    pairs, lists, total = packed.num_pairs, b * packed.num_pairs, packed.offsets[-1]
    x, k = f32(xyz), f32(intrinsics_px)
    pts = None if points_2d is None else f32(points_2d)
    ids_i, ids_j, wgt = packed.ids_i.contiguous(), packed.ids_j.contiguous(), f32(packed.weights)
    if ids_i.dtype != torch.int64 or ids_j.dtype != torch.int64:
        raise ValueError("pnp_ransac: the packed ids are int64")
    work = scratch(_lib.load().gsr_pnp_ransac_scratch_bytes(b, v, int(hypotheses)), torch.int64, dev)
    pairwise = torch.empty((b, pairs, 4, 4), dtype=torch.float32, device=dev)
    inliers = torch.empty(lists, dtype=torch.int32, device=dev)
    status = torch.empty(lists, dtype=torch.int32, device=dev)
    conf = torch.empty(lists, dtype=torch.float32, device=dev)
    mask = torch.empty(total, dtype=torch.uint8, device=dev) if return_mask else None
    n = len(packed.offsets)
    host = (ctypes.c_int32 * n)(*packed.offsets)
    launch("gsr_pnp_ransac", dev, b, v, h, w, pairs, x.data_ptr(), k.data_ptr(), ids_i.data_ptr(), ids_j.data_ptr(), wgt.data_ptr(), ptr(pts),
           host, packed.offsets_device.data_ptr(), int(hypotheses), float(reprojection_error), float(confidence_min),
           int(seed) & 0xffffffff, work.data_ptr(), pairwise.data_ptr(), inliers.data_ptr(), status.data_ptr(), conf.data_ptr(), ptr(mask))
    return pairwise, inliers, status, conf, mask


@torch.no_grad()
def pnp_ransac(xyz: Tensor, intrinsics_px: Tensor, packed: PackedCorrespondences, *, points_2d: Optional[Tensor] = None,
               hypotheses: int = 1000, reprojection_error: float = 5.0, seed: int = 0, return_mask: bool = False):
    """xyz (b, v, 3, h, w), pixel-unit intrinsics (b, v, 3, 3), the packed match lists -> (pairwise (b, P, 4, 4), inliers (P b,) int32,
    status (P b,) int32[, mask (M,) uint8]): per list the pose of the pair as the reference's `relpose` - the inverse of what
    cv2.solvePnPRansac returns for the second view's 3-D points and the first view's 2-D points -, P3P RANSAC over `hypotheses` draws
    and Gauss-Newton on the consensus set as include/gsr.h defines them; identity, 0 inliers and a status > 0 where there is no pose.
    `points_2d` (M, 2): sub-pixel keypoints (x, y) in the order of the pack; None: the pixel of `ids_i`.  Two launches, no host
    synchronisation; the same bits on every call with the same seed."""
    pairwise, inliers, status, _conf, mask = _pnp(xyz, intrinsics_px, packed, points_2d, hypotheses, reprojection_error, 0.5, seed, return_mask)
    return (pairwise, inliers, status, mask) if return_mask else (pairwise, inliers, status)


@torch.no_grad()
def synchronize_cameras(pairwise: Tensor, confidence: Tensor, num_views: int) -> Tensor:
    """pairwise (b, P, 4, 4), confidence (P b,) in list order (pair-major), the number of views -> (b, v, 4, 4): the reference's
    `camera_synchronization(Ps, confidence, v)` at its default arguments in one launch; a scene whose mass has a zero entry is
    chained, by itself (include/gsr.h)."""
    v = int(num_views)
    if v < 2 or v > MAX_VIEWS:
        raise ValueError(f"synchronize_cameras: needs 2 to {MAX_VIEWS} views, got {num_views}")
    pairs = v * (v - 1) // 2
    if pairwise.dim() != 4 or tuple(pairwise.shape[1:]) != (pairs, 4, 4):
        raise ValueError(f"synchronize_cameras: expected pairwise (b, {pairs}, 4, 4), got {tuple(pairwise.shape)}")
    b = pairwise.shape[0]
    if tuple(confidence.shape) != (pairs * b,):
        raise ValueError(f"synchronize_cameras: expected confidence (P b,) = ({pairs * b},), got {tuple(confidence.shape)}")
    require_device("pose", "synchronize_cameras", (pairwise, confidence))
    pw, cf = f32(pairwise), f32(confidence)
    out = torch.empty((b, v, 4, 4), dtype=torch.float32, device=pairwise.device)
    launch("gsr_camera_sync", pairwise.device, b, v, pw.data_ptr(), cf.data_ptr(), out.data_ptr())
    return out


@torch.no_grad()
def coarse_poses(xyz: Tensor, intrinsics_px: Tensor, packed: PackedCorrespondences, *, points_2d: Optional[Tensor] = None,
                 hypotheses: int = 1000, reprojection_error: float = 5.0, confidence_min: float = 0.5, seed: int = 0,
                 return_mask: bool = False) -> CoarsePoses:
    """The whole block: `pnp_ransac` per list, the lists' confidences (the mean score; for pairs of views that are not neighbours
    relu(c - confidence_min) / (1 - confidence_min); 0 for an empty list) and `synchronize_cameras`.  Three launches, no host
    synchronisation."""
    pairwise, inliers, status, conf, mask = _pnp(xyz, intrinsics_px, packed, points_2d, hypotheses, reprojection_error, confidence_min,
                                                 seed, return_mask)
    absolute = synchronize_cameras(pairwise, conf, xyz.shape[1])
    return CoarsePoses(pairwise, absolute, conf, inliers, status, mask)


class RefinedPoses(NamedTuple):
    c2w: Tensor  # (b, v, 4, 4): the reference's refine_sync_abspose
    w2c: Tensor  # (b, v, 4, 4): its .inverse()


class PoseErrors(NamedTuple):
    rotation: Tensor              # (b,) radians
    translation_angle: Tensor     # (b,) degrees
    translation_distance: Tensor  # (b,)


def pose_encoding(c2w: Tensor) -> Tensor:
    """(..., 4, 4) or (..., 3, 4) -> (..., 9): the reference's cat(matrix_to_rotation_6d(R), t) - rows 0 and 1 of the rotation, then the
    translation -, what `embed_pose` reads (encoder_costvolume.py:448-450, 453).  Plain torch indexing on any device."""
    if c2w.dim() < 2 or c2w.shape[-1] != 4 or c2w.shape[-2] not in (3, 4):
        raise ValueError(f"pose_encoding: expected poses (..., 4, 4), got {tuple(c2w.shape)}")
    return torch.cat([c2w[..., :2, :3].reshape(*c2w.shape[:-2], 6), c2w[..., :3, 3]], dim=-1)


def _delta_rows(delta: Tensor):
    """delta (b, v, 9) as the kernels read it: (tensor whose data_ptr is row (0, 0), floats per row).  Read where it lies if it is
    float32 with last stride 1 and uniform row strides (`full[..., :9]` of a contiguous (b, v, C)); anything else is copied once."""
    d = delta.detach()
    b, v, _ = d.shape
    if d.dtype == torch.float32 and d.stride(2) == 1:
        row = d.stride(1) if v > 1 else (d.stride(0) if b > 1 else 9)
        if row >= 9 and (b == 1 or d.stride(0) == v * row):
            return d, row
    return d.to(torch.float32).contiguous(), 9


def _refine_args(sync_abspose, delta, gamma):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if sync_abspose.dim() != 4 or tuple(sync_abspose.shape[2:]) != (4, 4):
        raise ValueError(f"refine_poses: expected sync_abspose (b, v, 4, 4), got {tuple(sync_abspose.shape)}")
    b, v = sync_abspose.shape[:2]
    if v < 1:
        raise ValueError(f"refine_poses: needs at least one view, got {v}")
    if delta.dim() != 3 or delta.shape[2] != 9:
        raise ValueError(f"refine_poses: expected delta (b, v, 9) - the first nine channels of the pose head's output -, got {tuple(delta.shape)}")
    if tuple(delta.shape[:2]) != (b, v):
        raise ValueError(f"refine_poses: sync_abspose is of (b, v) = ({b}, {v}), delta of {tuple(delta.shape[:2])}")
    if isinstance(gamma, Tensor) and gamma.numel() != 1:
        raise ValueError(f"refine_poses: expected gamma with one element, got {tuple(gamma.shape)}")
    tensors = [sync_abspose, delta] + ([gamma] if isinstance(gamma, Tensor) else [])
    require_device("pose", "refine_poses", tensors)
    return b, v


class _RefinePoses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sync_abspose, delta, gamma):
        b, v = _refine_args(sync_abspose, delta, gamma)
        rows, stride = _delta_rows(delta)
        if b * v * max(stride, 16) > 0x7fffffff:
            raise ValueError("refine_poses: more than 2^31 - 1 elements in the poses or in delta as strided")
        dev = sync_abspose.device
        sync = f32(sync_abspose)
        if isinstance(gamma, Tensor):
            g = gamma.detach().to(torch.float32).reshape(1)
        else:
            g = torch.full((1,), float(gamma), dtype=torch.float32, device=dev)
        c2w = torch.empty((b, v, 4, 4), dtype=torch.float32, device=dev)  # (both fully written by the call)
        w2c = torch.empty((b, v, 4, 4), dtype=torch.float32, device=dev)
        launch("gsr_pose_refine", dev, b, v, sync.data_ptr(), rows.data_ptr(), stride, g.data_ptr(), c2w.data_ptr(), w2c.data_ptr())
        ctx.save_for_backward(sync, delta, g)
        ctx.gamma_like = gamma if isinstance(gamma, Tensor) else None
        ctx.sizes = (b, v)
        ctx.set_materialize_grads(False)
        return c2w.to(sync_abspose.dtype), w2c.to(sync_abspose.dtype)

    @staticmethod
    def backward(ctx, g_c2w, g_w2c):
        sync, delta, g = ctx.saved_tensors
        b, v = ctx.sizes
        _, need_delta, need_gamma = ctx.needs_input_grad
        if not (need_delta or need_gamma) or (g_c2w is None and g_w2c is None) or b == 0:
            return None, None, None
        dev = sync.device
        rows, stride = _delta_rows(delta)
        ups = [None if t is None else f32(t) for t in (g_c2w, g_w2c)]
        d_delta = torch.empty((b, v, 9), dtype=torch.float32, device=dev) if need_delta else None  # (fully written by the call)
        d_gamma = torch.empty((1,), dtype=torch.float32, device=dev) if need_gamma else None
        launch("gsr_pose_refine_backward", dev, b, v, sync.data_ptr(), rows.data_ptr(), stride, g.data_ptr(), ptr(ups[0]), ptr(ups[1]),
               ptr(d_delta), ptr(d_gamma))
        like = ctx.gamma_like
        return (None, d_delta.to(delta.dtype) if need_delta else None,
                d_gamma.to(like.dtype).reshape(like.shape) if need_gamma else None)


def refine_poses(sync_abspose: Tensor, delta: Tensor, gamma) -> RefinedPoses:
    """sync_abspose (b, v, 4, 4) - `coarse_poses(...).absolute` -, delta (b, v, 9) - the first nine channels of the pose head's output -,
    gamma -> RefinedPoses(c2w, w2c), both (b, v, 4, 4), as include/gsr.h defines them: the pose as (rows 0 and 1 of R, t), plus
    gamma delta for every view but the first, Gram-Schmidt with F.normalize's clamp (the orthonormal vectors are the ROWS of R), and
    w2c = [R^T | -R^T t] - the reference's three `.inverse()` calls without an LU.  Differentiable in delta and in gamma; sync_abspose
    receives nothing (the reference's coarse poses come back from numpy).  The gradients are bit-reproducible (no atomics).
    delta is read where it lies when it is float32 with last stride 1 and uniform row strides - `pose_branch(...)[..., :9]`;
    anything else is copied once.  gamma: a 0-dim or one-element device tensor (the nn.Parameter), read on the device, or a Python
    float, which gets no gradient.  One launch each way, no host synchronisation.  Inputs that are not float32 are converted; results
    and gradients come back in the inputs' dtypes."""
    return RefinedPoses(*_RefinePoses.apply(sync_abspose, delta, gamma))


@torch.no_grad()
def pose_errors(c2w_pred: Tensor, extrinsics_gt: Tensor) -> PoseErrors:
    """c2w_pred (b, v, 4, 4) - `refine_poses(...).c2w` -, extrinsics_gt (b, v, 4, 4) - batch["context"]["extrinsics"] ->
    PoseErrors(rotation, translation_angle, translation_distance), each (b,), of the LAST view against gt_rel = E[:, -1]^-1 E[:, 0]
    (include/gsr.h): the geodesic angle in radians, the angle between the translation directions in degrees (NaN for a zero
    translation, as the reference's 0 / 0) and the distance of the translations.  The reference's three logged scalars
    (model_wrapper.py:182-190, 306-313, 345) are `rotation.mean()` (compute_geodesic_distance_from_two_matrices averages the batch),
    `translation_angle[0]` (its torch.dot takes scene 0) and `translation_distance[0]` at b = 1 (it calls `.item()` there).
    One launch, no gradient, no host synchronisation."""
    for name, t in (("c2w_pred", c2w_pred), ("extrinsics_gt", extrinsics_gt)):
        if t.dim() != 4 or tuple(t.shape[2:]) != (4, 4):
            raise ValueError(f"pose_errors: expected {name} (b, v, 4, 4), got {tuple(t.shape)}")
    b, v = c2w_pred.shape[:2]
    if v < 1:
        raise ValueError(f"pose_errors: needs at least one view, got {v}")
    if tuple(extrinsics_gt.shape[:2]) != (b, v):
        raise ValueError(f"pose_errors: c2w_pred is of (b, v) = ({b}, {v}), extrinsics_gt of {tuple(extrinsics_gt.shape[:2])}")
    if b * v * 16 > 0x7fffffff:
        raise ValueError("pose_errors: more than 2^31 - 1 elements in the poses")
    require_device("pose", "pose_errors", (c2w_pred, extrinsics_gt))
    pred, gt = f32(c2w_pred), f32(extrinsics_gt)
    out = torch.empty((3, b), dtype=torch.float32, device=c2w_pred.device)
    launch("gsr_pose_errors", c2w_pred.device, b, v, pred.data_ptr(), gt.data_ptr(), out.data_ptr())
    out = out.to(c2w_pred.dtype)
    return PoseErrors(out[0], out[1], out[2])
