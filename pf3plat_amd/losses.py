"""Photometric losses next to the raster path: counterparts of the reference's `LossMse`
(src/loss/loss_mse.py:23-36), `LossMultiSSIM` / `ssim` (src/loss/loss_multissim.py:24-83) and `compute_psnr`
(src/evaluation/metrics.py:11-19), all evaluated by ONE launch of the raster library (`gsr_image_loss`) that also writes
dL/dprediction in the layout the rasterizer's backward reads - the loss's backward is then a no-op (the gradient already
exists) instead of five depthwise convolutions and their transposes.  The evaluation's metrics - `compute_psnr` and `compute_ssim`
(src/evaluation/metrics.py:36-52: scikit-image's structural_similarity, another SSIM than the loss's) - come from a launch pair of
their own (`gsr_image_metrics`, forward only).  The fourth loss of the training step, `Losspose` (src/loss/loss_pose.py:28-129), is
`pose_loss` / `Losspose` at the end of this file: one launch chain in each direction (`gsr_pose_loss`, `gsr_pose_loss_backward`)
instead of a Python loop over the (scene, pair) lists.  The perceptual term, `LossLpips` (src/loss/loss_lpips.py), and the
evaluation's `compute_lpips` (src/evaluation/metrics.py:27-33) follow it: the VGG convolutions in torch, the distance head in
pf3plat_amd.lpips.  No CPU fallback: tensors must be on a ROCm device.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._call import call, f32, launch, ptr, require_device
from .rasterizer import _on_device, _stream_ptr


def _launch(prediction: Tensor, target: Tensor, mse_weight: float, ssim_weight: float, want_grad: bool):
    """-> (sums (n, 4): per image squared error, clipped squared error, SSIM map, 0; totals (4,): loss, mse, mean ssim, 0;
    dL/dprediction or None; elements per image).  Two launches (gsr_image_loss, gsr_image_loss_finish), no torch op."""
    require_device("losses", "photometric_loss", (prediction, target))
    if prediction.shape != target.shape or prediction.dim() != 4 or prediction.shape[1] != 3:
        raise ValueError(f"expected two (n, 3, h, w) images, got {tuple(prediction.shape)} and {tuple(target.shape)}")
    lib = _lib.load()
    pred, tgt = f32(prediction), f32(target)
    n, _, h, w = pred.shape
    dev = pred.device
    if n == 0:
        z = torch.zeros((1, 4), dtype=torch.float32, device=dev)
        return z[:0], z[0], (torch.empty_like(pred) if want_grad else None), 3 * h * w
    slots = int(lib.gsr_image_loss_partials(n, h, w))
    partials = torch.empty((slots, 4), dtype=torch.float32, device=dev)
    out = torch.empty((n + 1, 4), dtype=torch.float32, device=dev)  # the images' sums, then the batch's totals
    grad = torch.empty_like(pred) if want_grad else None
    stream = _stream_ptr(dev)
    pp = partials.data_ptr()
    with _on_device(dev):
        call("gsr_image_loss", stream, n, h, w, pred.data_ptr(), tgt.data_ptr(), float(mse_weight), float(ssim_weight), ptr(grad), pp)
        call("gsr_image_loss_finish", stream, n, h, w, pp, float(mse_weight), float(ssim_weight), out.data_ptr(), out[n].data_ptr())
    return out[:n], out[n], grad, 3 * h * w


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, target, mse_weight, ssim_weight):
        _sums, totals, grad, _per_image = _launch(prediction, target, mse_weight, ssim_weight, prediction.requires_grad)
        ctx.grad = grad
        loss, mse, ssim = totals[0], totals[1], totals[2]
        ctx.mark_non_differentiable(mse, ssim)
        return loss, mse, ssim

    @staticmethod
    def backward(ctx, g_loss, _g_mse, _g_ssim):
        return (None if ctx.grad is None else ctx.grad * g_loss), None, None, None


def photometric_loss(prediction: Tensor, target: Tensor, mse_weight: float = 1.0, ssim_weight: float = 0.0):
    """prediction, target (n, 3, h, w) -> (loss, mse, mean ssim) with loss = mse_weight * mse + ssim_weight * (1 - mean ssim);
    differentiable in `prediction` (the gradient is produced by the same launch)."""
    return _Photometric.apply(prediction, target, float(mse_weight), float(ssim_weight))


def ssim(img1: Tensor, img2: Tensor) -> Tensor:
    """Mean SSIM map of two (n, 3, h, w) batches (the reference's `ssim(img1, img2)` with its defaults)."""
    return photometric_loss(img1, img2, 0.0, -1.0)[0] + 1.0  # loss = -(1 - ssim)


@torch.no_grad()
def compute_psnr(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """(batch, 3, h, w) x 2 -> (batch,): -10 log10 of the mean squared error of the inputs clipped to [0, 1]."""
    sums, _totals, _, per_image = _launch(predicted, ground_truth, 0.0, 0.0, False)
    return -10 * (sums[:, 1] / per_image).log10()


def _launch_metrics(ground_truth: Tensor, predicted: Tensor, want_map: bool):
    """-> (metrics (4, n): per image SSIM, PSNR, interior sum of the SSIM map, clipped squared error; the map (n, 3, h, w) or None).
    Two launches (gsr_image_metrics, gsr_image_metrics_finish), no torch op.  The shapes are checked first, before the device and
    before the library is loaded."""
    if ground_truth.shape != predicted.shape or ground_truth.dim() != 4 or ground_truth.shape[1] != 3:
        raise ValueError(f"expected two (n, 3, h, w) images, got {tuple(ground_truth.shape)} and {tuple(predicted.shape)}")
    n, _, h, w = ground_truth.shape
    if h < 11 or w < 11:
        raise ValueError(f"win_size exceeds image extent: the 11 x 11 window of compute_ssim needs h, w >= 11, got {h} x {w}")
    require_device("losses", "compute_image_metrics", (ground_truth, predicted))
    lib = _lib.load()
    gt, pred = f32(ground_truth), f32(predicted)
    dev = gt.device
    out = torch.empty((4, n), dtype=torch.float32, device=dev)
    smap = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if want_map else None
    if n == 0:
        return out, smap
    slots = int(lib.gsr_image_metrics_partials(n, h, w))
    if slots == 0:
        raise RuntimeError(f"gsr_image_metrics takes at most 21845 images in one call, got {n}")
    partials = torch.empty((slots, 4), dtype=torch.float32, device=dev)
    stream = _stream_ptr(dev)
    with _on_device(dev):
        call("gsr_image_metrics", stream, n, h, w, gt.data_ptr(), pred.data_ptr(), ptr(smap), partials.data_ptr())
        call("gsr_image_metrics_finish", stream, n, h, w, partials.data_ptr(), out.data_ptr())
    return out, smap


@torch.no_grad()
def compute_image_metrics(ground_truth: Tensor, predicted: Tensor, ssim_map: bool = False):
    """(batch, 3, h, w) x 2 -> (psnr (batch,), ssim (batch,)[, map (batch, 3, h, w)]): the reference's compute_psnr and compute_ssim
    (src/evaluation/metrics.py:11-19, 36-52) from one launch pair, without a host synchronisation; `ssim_map`: also the SSIM map
    on every pixel (scikit-image's `full=True`), border included.  h, w >= 11."""
    out, smap = _launch_metrics(ground_truth, predicted, ssim_map)
    return (out[1], out[0], smap) if ssim_map else (out[1], out[0])


@torch.no_grad()
def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """(batch, 3, h, w) x 2 -> (batch,): per image skimage.metrics.structural_similarity(gt, hat, win_size=11, gaussian_weights=True,
    channel_axis=0, data_range=1.0) - reflected borders, sample covariance, mean over the interior without its 5-pixel border, mean
    of the three channels (include/gsr.h states the definition).  NOT `ssim` above, which is the training loss's."""
    return _launch_metrics(ground_truth, predicted, False)[0][0]


@dataclass
class LossMseCfg:
    weight: float


@dataclass
class LossMultiSSIMCfg:
    weight: float


def _inner_views(prediction_color: Tensor, batch) -> tuple:
    """The reference compares the target views without the first and the last one ([:, 1:-1]); (b, v, 3, h, w) -> (b v, 3, h, w)."""
    pred = prediction_color[:, 1:-1]
    tgt = batch["target"]["image"][:, 1:-1]
    return pred.reshape(-1, *pred.shape[2:]), tgt.reshape(-1, *tgt.shape[2:])


class LossMse(torch.nn.Module):
    """`forward(prediction, batch, ...)` as the reference's LossMse: weight x mean squared error over the inner target views."""

    def __init__(self, cfg: LossMseCfg):
        super().__init__()
        self.cfg = cfg

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0, *unused) -> Tensor:
        return photometric_loss(*_inner_views(prediction.color, batch), self.cfg.weight, 0.0)[0]


class LossMultiSSIM(torch.nn.Module):
    """`forward(prediction, batch, ...)` as the reference's LossMultiSSIM: weight x (1 - mean SSIM) over the inner target views."""

    def __init__(self, cfg: LossMultiSSIMCfg):
        super().__init__()
        self.cfg = cfg

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0, *unused) -> Tensor:
        return photometric_loss(*_inner_views(prediction.color, batch), 0.0, self.cfg.weight)[0]


class LossPhotometric(torch.nn.Module):
    """Both terms from one launch (what a training step that uses the two reference losses together should call)."""

    def __init__(self, mse: Optional[LossMseCfg] = None, ssim: Optional[LossMultiSSIMCfg] = None):
        super().__init__()
        self.mse_weight = 0.0 if mse is None else mse.weight
        self.ssim_weight = 0.0 if ssim is None else ssim.weight

    def forward(self, prediction, batch, *unused) -> Tensor:
        return photometric_loss(*_inner_views(prediction.color, batch), self.mse_weight, self.ssim_weight)[0]


# ------------------------------------------------------------------------------------------------------------------------
# The pose loss (reference src/loss/loss_pose.py; the definition is stated in include/gsr.h)
# ------------------------------------------------------------------------------------------------------------------------
@dataclass
class PackedCorrespondences:
    """The match lists of one batch as the kernels read them: list l = pair x num_scenes + scene (pair-major, pairs in the order
    [(a, c) for a in range(v) for c in range(a + 1, v)]) holds entries offsets[l] .. offsets[l + 1] of the three arrays."""
    ids_i: Tensor           # (M,) int64 flat pixel indices y * w + x in the pair's first view
    ids_j: Tensor           # (M,) int64, in its second view
    weights: Tensor         # (M,) float32 scores
    conf: Tensor            # (num_pairs * num_scenes,) float32, one confidence per list
    offsets: tuple          # num_lists + 1 Python ints (from the shapes: nothing is read off the device)
    offsets_device: Tensor  # the same as int32 on the arrays' device
    num_scenes: int
    num_pairs: int


def pack_correspondences(corr, conf) -> PackedCorrespondences:
    """The reference's `corr[0]` - {(i, j): [(id_i, id_j, score) per scene]} - and `corr[2]` - {(i, j): one confidence per scene} -
    as four arrays: one `torch.cat` each, in the order the reference indexes them, the offsets from the shapes (no synchronisation:
    on a device the offsets go up from pinned memory without waiting).  Neither scores nor confidences carry a gradient.  Ids outside
    [0, h * w) are the caller's error: nobody checks them per match, here or in the kernels."""
    pairs = sorted(corr.keys())
    if not pairs:
        raise ValueError("pack_correspondences: no pairs")
    num_views = max(j for _, j in pairs) + 1
    if pairs != [(a, c) for a in range(num_views) for c in range(a + 1, num_views)]:
        raise ValueError(f"pack_correspondences: expected every pair (i, j), i < j, of {num_views} views, got {pairs}")
    num_scenes = len(corr[pairs[0]])
    if any(len(corr[p]) != num_scenes or len(conf[p]) != num_scenes for p in pairs):
        raise ValueError("pack_correspondences: every pair needs one list and one confidence per scene")
    lists = [corr[p][s] for p in pairs for s in range(num_scenes)]
    offsets = [0]
    for ids_i, ids_j, score in lists:
        if not (ids_i.dim() == ids_j.dim() == score.dim() == 1 and ids_i.shape == ids_j.shape == score.shape):
            raise ValueError(f"pack_correspondences: a list is three equal 1-D tensors, got {tuple(ids_i.shape)}, {tuple(ids_j.shape)}, {tuple(score.shape)}")
        offsets.append(offsets[-1] + ids_i.shape[0])
    if offsets[-1] > 0x7fffffff:
        raise ValueError("pack_correspondences: more than 2^31 - 1 matches in one call")
    ids_i = torch.cat([t[0] for t in lists]).detach().to(torch.int64)
    ids_j = torch.cat([t[1] for t in lists]).detach().to(torch.int64)
    weights = torch.cat([t[2] for t in lists]).detach().to(torch.float32)
    dev = weights.device
    cf = torch.cat([(conf[p] if isinstance(conf[p], Tensor) else torch.stack([torch.as_tensor(c, device=dev) for c in conf[p]])).reshape(-1) for p in pairs])
    cf = cf.detach().to(device=dev, dtype=torch.float32)
    off = torch.tensor(offsets, dtype=torch.int32)
    off = off.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else off
    return PackedCorrespondences(ids_i, ids_j, weights, cf, tuple(offsets), off, num_scenes, len(pairs))


def _pose_loss_args(xyz, depth, poses, intrinsics, packed):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if xyz.dim() != 5 or xyz.shape[2] != 3:
        raise ValueError(f"pose_loss: expected xyz (b, v, 3, h, w), got {tuple(xyz.shape)}")
    b, v, _, h, w = xyz.shape
    if v < 2:
        raise ValueError(f"pose_loss: needs at least two views, got {v}")
    if tuple(depth.shape) not in ((b * v, 1, h, w), (b, v, h, w)):
        raise ValueError(f"pose_loss: expected depth ((b v), 1, h, w) or (b, v, h, w) = ({b * v}, 1, {h}, {w}), got {tuple(depth.shape)}")
    if tuple(poses.shape) != (b, v, 4, 4):
        raise ValueError(f"pose_loss: expected poses (b, v, 4, 4) = ({b}, {v}, 4, 4), got {tuple(poses.shape)}")
    if tuple(intrinsics.shape) != (b, v, 3, 3):
        raise ValueError(f"pose_loss: expected intrinsics (b, v, 3, 3) = ({b}, {v}, 3, 3), got {tuple(intrinsics.shape)}")
    if packed.num_scenes != b or packed.num_pairs != v * (v - 1) // 2 or len(packed.offsets) != b * packed.num_pairs + 1:
        raise ValueError(f"pose_loss: the correspondences are packed for {packed.num_scenes} scenes and {packed.num_pairs} pairs, "
                         f"the points are of {b} scenes and {v} views ({v * (v - 1) // 2} pairs)")
    require_device("losses", "pose_loss", (xyz, depth, poses, intrinsics, packed.ids_i, packed.ids_j, packed.weights, packed.conf,
                                           packed.offsets_device))
    return b, v, h, w


def _pose_call(name, b, v, h, w, packed, arrays, weight_2d, weight_3d, tail, dev):
    n = len(packed.offsets)
    host = (ctypes.c_int32 * n)(*packed.offsets)
    launch(name, dev, b, v, h, w, packed.num_pairs, *(t.data_ptr() for t in arrays), packed.ids_i.data_ptr(), packed.ids_j.data_ptr(),
           packed.weights.data_ptr(), packed.conf.data_ptr(), host, packed.offsets_device.data_ptr(), weight_2d, weight_3d,
           *(t.data_ptr() for t in tail))


def _pose_units(lib, packed) -> int:
    n = len(packed.offsets)
    units = int(lib.gsr_pose_loss_units(n - 1, (ctypes.c_int32 * n)(*packed.offsets)))
    if units < 0:
        raise RuntimeError("gsr_pose_loss_units refused the offsets")
    return units


class _PoseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, depth, poses, intrinsics, packed, weight_2d, weight_3d):
        b, v, h, w = _pose_loss_args(xyz, depth, poses, intrinsics, packed)
        lib = _lib.load()
        dev = xyz.device
        arrays = (f32(xyz), f32(depth), f32(poses), f32(intrinsics))
        units = _pose_units(lib, packed)
        partials = torch.empty((max(units, 1), 4), dtype=torch.float32, device=dev)
        lists = torch.empty((max(b * packed.num_pairs, 1), 4), dtype=torch.float32, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        _pose_call("gsr_pose_loss", b, v, h, w, packed, arrays, weight_2d, weight_3d, (partials, lists, out), dev)
        ctx.save_for_backward(xyz, depth, poses, intrinsics, lists)
        ctx.call = (b, v, h, w, packed, weight_2d, weight_3d, units)
        loss, loss_3d, loss_2d = out[0], out[1], out[2]
        ctx.mark_non_differentiable(loss_3d, loss_2d)
        return loss, loss_3d, loss_2d

    @staticmethod
    def backward(ctx, g_loss, _g_3d, _g_2d):
        xyz, depth, poses, intrinsics, lists = ctx.saved_tensors
        b, v, h, w, packed, weight_2d, weight_3d, units = ctx.call
        dev = xyz.device
        arrays = (f32(xyz), f32(depth), f32(poses), f32(intrinsics))
        d_xyz = torch.empty((b, v, 3, h, w), dtype=torch.float32, device=dev)  # (zero-filled by the call)
        d_depth = torch.empty((b, v, h, w), dtype=torch.float32, device=dev)
        d_poses = torch.empty((b, v, 4, 4), dtype=torch.float32, device=dev)
        partials = torch.empty((max(units, 1), 12), dtype=torch.float32, device=dev)
        up = f32(g_loss).reshape(1)
        _pose_call("gsr_pose_loss_backward", b, v, h, w, packed, arrays, weight_2d, weight_3d, (lists, up, d_xyz, d_depth, d_poses, partials), dev)
        need = ctx.needs_input_grad
        return (d_xyz.to(xyz.dtype) if need[0] else None, d_depth.reshape(depth.shape).to(depth.dtype) if need[1] else None,
                d_poses.to(poses.dtype) if need[2] else None, None, None, None, None)


def pose_loss(xyz: Tensor, depth: Tensor, poses: Tensor, intrinsics: Tensor, packed: PackedCorrespondences, weight_2d: float, weight_3d: float):
    """xyz (b, v, 3, h, w), depth ((b v), 1, h, w) or (b, v, h, w), poses (b, v, 4, 4) (the top three rows are read), normalised
    intrinsics (b, v, 3, 3), the packed match lists -> (loss, mean 3D term, mean 2D term), loss = weight_3d x mean 3D + weight_2d x
    mean 2D as include/gsr.h defines them; differentiable in xyz, depth and poses (the two means are for logging).  Two launches
    forward, a zero-fill and two launches backward, no host synchronisation either way.  Inputs that are not float32 or not
    contiguous are converted.  Ids outside [0, h * w) are the caller's error and are NOT checked per match."""
    return _PoseLoss.apply(xyz, depth, poses, intrinsics, packed, float(weight_2d), float(weight_3d))


@dataclass
class LossposeCfg:
    weight_2d: float
    weight_3d: float


class Losspose(torch.nn.Module):
    """`forward(prediction, batch, gaussians, global_step, c2w, depth, corr, xyz_h)` as the reference's Losspose: it reads
    batch["target"]["intrinsics"], the learned poses c2w[1], the refined depth depth[0], the matches corr[0] with their confidences
    corr[2] and the refined points xyz_h, and ignores c2w[0] (the reference computes a second pair of terms from it and drops them)."""

    def __init__(self, cfg: LossposeCfg):
        super().__init__()
        self.cfg = cfg

    def forward(self, prediction, batch, gaussians, global_step, c2w, depth, corr, xyz_h) -> Tensor:
        packed = pack_correspondences(corr[0], corr[2])
        return pose_loss(xyz_h, depth[0], c2w[1], batch["target"]["intrinsics"], packed, self.cfg.weight_2d, self.cfg.weight_3d)[0]


# ------------------------------------------------------------------------------------------------------------------------
# The perceptual term (reference src/loss/loss_lpips.py, src/evaluation/metrics.py:21-33; the definition is stated in include/gsr.h)
# ------------------------------------------------------------------------------------------------------------------------
@dataclass
class LossLpipsCfg:
    weight: float
    apply_after_step: int


class LossLpips(torch.nn.Module):
    """`forward(prediction, batch, gaussians, global_step, ...)` as the reference's LossLpips: weight x the mean perceptual distance
    (`lpips.LPIPS`, normalize=True) over the inner target views; before `apply_after_step` a zero tensor, with no launch.  `lpips`:
    the network (pf3plat_amd.lpips.LPIPS); without one, or a `state_dict` for one, it holds seeded random weights - see there."""

    def __init__(self, cfg: LossLpipsCfg, lpips=None, state_dict=None):
        super().__init__()
        from .lpips import LPIPS

        self.cfg = cfg
        self.lpips = lpips if lpips is not None else LPIPS(state_dict)

    def forward(self, prediction, batch, gaussians=None, global_step: int = 0, *unused) -> Tensor:
        image = batch["target"]["image"]
        if global_step < self.cfg.apply_after_step:
            return torch.tensor(0, dtype=torch.float32, device=image.device)
        pred, tgt = _inner_views(prediction.color, batch)
        return self.cfg.weight * self.lpips(pred, tgt, normalize=True).mean()


_lpips_models = {}


@torch.no_grad()
def compute_lpips(ground_truth: Tensor, predicted: Tensor, lpips=None, state_dict=None) -> Tensor:
    """(batch, 3, h, w) x 2 in [0, 1] -> (batch,): the reference's compute_lpips, `LPIPS(ground_truth, predicted, normalize=True)[:, 0, 0, 0]`
    without a gradient.  `lpips`: the network; without one, one module per device is made on first use and kept, as the reference's
    cached `get_lpips`.  `state_dict`: the package's weights for that cached module (pf3plat_amd.lpips.LPIPS; given again, it is loaded
    again).  A cached module made WITHOUT a state dict holds seeded random weights, its numbers are not the published metric's, and
    making it warns once per device."""
    if lpips is None:
        require_device("losses", "compute_lpips", (ground_truth, predicted))
        lpips = _lpips_models.get(predicted.device)
        if lpips is None:
            from .lpips import LPIPS

            if state_dict is None:
                import warnings

                warnings.warn("compute_lpips: no network and no state dict given - the cached LPIPS module holds seeded RANDOM weights and "
                              "its values are not the published metric's; pass lpips= or state_dict= (pf3plat_amd.lpips.LPIPS)", stacklevel=2)
            lpips = _lpips_models[predicted.device] = LPIPS(state_dict).to(predicted.device)
        elif state_dict is not None:
            lpips.load_lpips_state_dict(state_dict)
    return lpips(ground_truth, predicted, normalize=True)[:, 0, 0, 0]
