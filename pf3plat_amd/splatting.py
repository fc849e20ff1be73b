"""Host wrappers of the rasterizer: counterparts of the reference's
src/model/decoder/cuda_splatting.py (`render_cuda` :47-127, `render_cuda_orthographic` :130-220,
`render_depth_cuda` :226-269) with the same names, argument meaning and results.

What differs is how the device is driven, not what is computed:
  * the reference loops over views in Python, with two `.item()` host syncs and one rasterizer
    invocation per view (:91-126); here all `batch` views go through ONE launch chain
    (`rasterize_views`), camera parameters never leave the device;
  * the scale-invariant pre-scale of means/covariances (:64-71) is not materialised: the factor
    travels in the per-view camera record and is applied on load inside the kernels (same fp32
    multiplies), and its chain rule is applied inside the backward kernel;
  * `render_views` (below) additionally shares one copy of the Gaussians between all views of a
    scene and blends the depth image as a 4th channel of the same pass.
"""
from __future__ import annotations

from math import isqrt
from typing import Optional

import torch
from torch import Tensor

from .rasterizer import get_backend, rasterize_views, views_from_cameras
from .types import DepthRenderingMode


def _viewbuf(extrinsics, intrinsics, near, far, background_color, scale_invariant: bool, pose_gradients: bool = False,
             intrinsics_gradients: bool = False) -> Tensor:
    """Camera records for `rasterize_views`: the arithmetic of the reference wrapper at cuda_splatting.py:64-71 / :80-87
    (1 / near rescale, get_fov, get_projection_matrix, extrinsics.inverse(), view @ proj) in ONE launch of the raster
    library (`gsr_setup_views`), straight into the records the kernels read.  Cameras carry no gradient (settings object)
    unless pose_gradients (to `extrinsics`) or intrinsics_gradients (to `intrinsics`) asks for one."""
    return views_from_cameras(extrinsics, intrinsics, near, far, background_color, scale_invariant, pose_gradients, intrinsics_gradients)


def depth_fake_color(extrinsics: Tensor, near: Tensor, far: Tensor, gaussian_means: Tensor, mode: DepthRenderingMode) -> Tensor:
    """The scalar the reference's depth render blends, as differentiable torch ops (cuda_splatting.py:238-251,
    conversions.py:17-27): camera-space z of every mean in UN-normalised units, mapped by `mode`.  extrinsics (V, 4, 4),
    near / far (V,), gaussian_means (S, G, 3) with V = S x views_per_set (set-major) -> (V, G).  The kernels evaluate the same
    f(z) themselves (GSR_FLAG_EXTRA_MODE) and, since round 4, return the camera's share of its gradient too (the reference's
    graph reaches `extrinsics` through `extrinsics.inverse()` here - the one place a camera gets any): nothing in the package
    calls this any more; it stays as the torch statement of that graph, which the tests differentiate with autograd to check
    the fused path (tests/test_gpu_api.py, tests/test_wrappers_cpu.py)."""
    v, s = extrinsics.shape[0], gaussian_means.shape[0]
    row = extrinsics.inverse()[:, 2, :]  # world -> camera z
    m = gaussian_means if v == s else gaussian_means.repeat_interleave(v // s, dim=0)
    z = (m * row[:, None, :3]).sum(-1) + row[:, None, 3]
    if mode == "disparity":
        return 1 / z
    if mode == "relative_disparity":
        eps = 1e-10
        disp_near, disp_far = 1 / (near[:, None] + eps), 1 / (far[:, None] + eps)
        return 1 - (1 / (z + eps) - disp_far) / (disp_near - disp_far + eps)
    if mode == "log":  # (the reference's min(near).max(far) is the constant log(far): kept)
        return z.minimum(near[:, None]).maximum(far[:, None]).log()
    return z


def _scale_rot_records(scales: Tensor, rotations: Tensor) -> Tensor:
    """(..., 7) scale + quaternion records for the raster kernels.  When `scales` and `rotations` are the two slices [..., :3] and
    [..., 3:] of one contiguous (..., 7) tensor - what GaussianAdapter(fused=True) returns, also after `for_decoder`'s reshapes - that
    tensor is passed on as it is (same values, one copy fewer in each direction); anything else is concatenated."""
    base = scales._base
    lead = tuple(scales.shape[:-1])
    if (base is not None and rotations._base is base and base.dim() >= 1 and base.shape[-1] == 7 and base.is_contiguous()
            and scales.shape[-1] == 3 and rotations.shape[-1] == 4 and tuple(rotations.shape[:-1]) == lead
            and base.numel() == 7 * scales.numel() // 3 and scales.dtype == base.dtype
            and scales.storage_offset() == base.storage_offset() and rotations.storage_offset() == base.storage_offset() + 3):
        want, step = [], 7  # the strides a (*lead, 7) view of the whole of `base` gives both slices
        for size in reversed(lead):
            want.append(step)
            step *= size
        want = tuple(reversed(want)) + (1,)
        same = lambda t: all(sz == 1 or st == w for sz, st, w in zip(t.shape, t.stride(), want))
        if same(scales) and same(rotations):
            return base.view(*lead, 7)
    return torch.cat((scales, rotations), dim=-1)


def _camera_wants_depth_gradient(extrinsics: Tensor) -> bool:
    return torch.is_grad_enabled() and extrinsics.requires_grad


def render_cuda(
    extrinsics: Tensor,  # (batch, 4, 4) camera-to-world
    intrinsics: Tensor,  # (batch, 3, 3) normalised
    near: Tensor,  # (batch,)
    far: Tensor,  # (batch,)
    image_shape: tuple,
    background_color: Tensor,  # (batch, 3)
    gaussian_means: Tensor,  # (batch, gaussian, 3)
    gaussian_covariances: Tensor,  # (batch, gaussian, 3, 3)
    gaussian_sh_coefficients: Tensor,  # (batch, gaussian, 3, d_sh)
    gaussian_opacities: Tensor,  # (batch, gaussian)
    scale_invariant: bool = True,
    use_sh: bool = True,
    intrinsics_gradients: bool = False,  # opt-in: the render's gradient reaches `intrinsics` (the reference's does not)
) -> Tensor:  # (batch, 3, height, width)
    assert use_sh or gaussian_sh_coefficients.shape[-1] == 1
    viewbuf = _viewbuf(extrinsics, intrinsics, near, far, background_color, scale_invariant, False, intrinsics_gradients)
    _, _, _, n = gaussian_sh_coefficients.shape
    degree = isqrt(n) - 1
    # harmonics (b, g, 3, d_sh) and covariances (b, g, 3, 3) go to the operator as they are (no re-layout copies;
    # the reference permutes + gathers here, cuda_splatting.py:75,115,123)
    colors = gaussian_sh_coefficients if use_sh else gaussian_sh_coefficients[:, :, :, 0]
    color, _, _ = rasterize_views(
        gaussian_means, gaussian_covariances, gaussian_opacities, colors, viewbuf,
        image_shape=image_shape, sh_degree=degree, use_sh=use_sh, views_per_set=1, sh_planar=True, cov_3x3=True,
        intrinsics_gradients=intrinsics_gradients)
    return color


def render_cuda_orthographic(
    extrinsics: Tensor,  # (batch, 4, 4)
    width: Tensor,  # (batch,)
    height: Tensor,  # (batch,)
    near: Tensor,
    far: Tensor,
    image_shape: tuple,
    background_color: Tensor,  # (batch, 3)
    gaussian_means: Tensor,
    gaussian_covariances: Tensor,
    gaussian_sh_coefficients: Tensor,
    gaussian_opacities: Tensor,
    fov_degrees: float = 0.1,
    use_sh: bool = True,
    dump: Optional[dict] = None,
) -> Tensor:
    """Fake orthographic projection: camera moved back, tiny field of view (reference :130-220).
    Keeps the reference's `fov_y = atan(2 tan_fov_y)` quirk (:160)."""
    assert use_sh or gaussian_sh_coefficients.shape[-1] == 1
    _, _, _, n = gaussian_sh_coefficients.shape
    degree = isqrt(n) - 1
    with torch.no_grad():
        viewbuf, moved = get_backend().setup_views_orthographic(extrinsics, width, height, near, far, background_color,
                                                                float(fov_degrees))
    if dump is not None:
        dump.update(moved)  # extrinsics (b, 4, 4) after the move, fov_x (scalar), fov_y / near / far (b,)
    # harmonics (b, g, 3, d_sh) and covariances (b, g, 3, 3) go to the operator as they are (as in render_cuda)
    colors = gaussian_sh_coefficients if use_sh else gaussian_sh_coefficients[:, :, :, 0]
    color, _, _ = rasterize_views(
        gaussian_means, gaussian_covariances, gaussian_opacities, colors, viewbuf,
        image_shape=image_shape, sh_degree=degree, use_sh=use_sh, views_per_set=1, sh_planar=True, cov_3x3=True)
    return color


def render_depth_cuda(
    extrinsics: Tensor,
    intrinsics: Tensor,
    near: Tensor,
    far: Tensor,
    image_shape: tuple,
    gaussian_means: Tensor,
    gaussian_covariances: Tensor,
    gaussian_opacities: Tensor,
    scale_invariant: bool = True,
    mode: DepthRenderingMode = "depth",
    gaussian_scales: Optional[Tensor] = None,  # } instead of gaussian_covariances (pass None there): the adapter's
    gaussian_rotations: Optional[Tensor] = None,  # } scale + quaternion (x, y, z, w) form, covariance built in the kernels
    frames: Optional[Tensor] = None,
) -> Tensor:  # (batch, height, width)
    """Depth image = sum_i f(z_i) alpha_i T_i (reference :226-269).  The reference renders f(z) as a
    3-channel precomputed colour and averages the channels; the three channels are identical, so it
    is blended here once, as the extra channel of a colour-less pass, with f(z) evaluated inside the
    kernels.  Gaussians receive the same gradients as in the reference.  When `extrinsics` requires grad
    the reference's torch graph also sends a gradient to the camera through `extrinsics.inverse()`
    (:239-242; in training the extrinsics come from the encoder, model_wrapper.py:148-150): f(z) is then
    formed by `depth_fake_color` in torch and blended as an explicit extra channel, so that autograd
    carries exactly that gradient (means and camera); otherwise no torch op touches the Gaussians.

    `gaussian_*` may hold ONE copy of the Gaussians per scene while the cameras hold `views_per_scene` views per scene
    (batch = scenes x views_per_scene, scene-major): the views of a scene then share that copy, as in `render_views`."""
    b = extrinsics.shape[0]
    sets, g = gaussian_opacities.shape
    if b % max(sets, 1) != 0:
        raise ValueError(f"{b} cameras cannot be split over {sets} Gaussian sets")
    dev = gaussian_means.device
    # (extrinsics requiring grad: the camera records carry a gradient path, and the backward returns the depth term's share of it)
    cam_grad = _camera_wants_depth_gradient(extrinsics)
    viewbuf = _viewbuf(extrinsics, intrinsics, near, far, torch.zeros(3, dtype=torch.float32, device=dev), scale_invariant, cam_grad)
    # no colour is wanted: one shared zero colour row per set costs nothing to blend next to the depth channel
    zero_rgb = torch.zeros((1, 1, 3), dtype=torch.float32, device=dev).expand(sets, g, 3)
    channel = dict(extra_mode=mode, camera_gradient="depth")
    if gaussian_covariances is None:
        cov = dict(scale_rot=True, frames=frames)
        gaussian_covariances = _scale_rot_records(gaussian_scales, gaussian_rotations)
    else:
        cov = dict(cov_3x3=True)
    _, depth, _ = rasterize_views(
        gaussian_means, gaussian_covariances, gaussian_opacities, zero_rgb, viewbuf,
        image_shape=image_shape, sh_degree=0, use_sh=False, views_per_set=b // max(sets, 1), **channel, **cov)
    return depth


def render_views(
    extrinsics: Tensor,  # (scene, view, 4, 4)
    intrinsics: Tensor,  # (scene, view, 3, 3)
    near: Tensor,  # (scene, view)
    far: Tensor,  # (scene, view)
    image_shape: tuple,
    background_color: Tensor,  # (3,)
    gaussian_means: Tensor,  # (scene, gaussian, 3)
    gaussian_covariances: Tensor,  # (scene, gaussian, 3, 3)
    gaussian_sh_coefficients: Tensor,  # (scene, gaussian, 3, d_sh)
    gaussian_opacities: Tensor,  # (scene, gaussian)
    depth_mode: Optional[DepthRenderingMode] = None,
    scale_invariant: bool = True,
    gaussian_scales: Optional[Tensor] = None,  # (scene, gaussian, 3)   } instead of gaussian_covariances (pass None there):
    gaussian_rotations: Optional[Tensor] = None,  # (scene, gaussian, 4) } the covariance is built inside the kernels
    frames: Optional[Tensor] = None,  # (scene, F, 3, 3) world rotation per group of gaussian / F consecutive Gaussians
    pose_gradients: bool = False,  # opt-in: the render's gradient reaches `extrinsics` (the reference's does not)
    sh_frame: Optional[str] = None,  # "e3nn" | "rasterizer": the harmonics are in the coordinates of `frames` (rasterize_views)
    alpha: bool = False,  # also return the accumulated opacity A = 1 - T_final of every pixel (rasterize_views(return_alpha=True))
    intrinsics_gradients: bool = False,  # opt-in: the render's gradient reaches `intrinsics` (focal lengths, principal point)
):
    """Fused decoder path: all views of all scenes in one launch chain, Gaussians read once per scene
    (no V-fold `repeat`, reference decoder_splatting_cuda.py:52-56), depth as a 4th blended channel.
    Returns (color (scene, view, 3, h, w), depth (scene, view, h, w) | None) and, with alpha=True, a third element: the accumulated
    opacity (scene, view, h, w), differentiable like the other two.  The depth the reference blends is un-normalised (sum z alpha T);
    the expected depth of a pixel is depth / alpha, from this one pass - how to clamp a small alpha is the caller's choice.
    intrinsics_gradients: when `intrinsics` requires grad it receives the render's gradient - the full camera gradient of the records
    with its tan-fov columns (GSR_FLAG_FOV_GRADIENT), carried through the set-up's arithmetic.  `extrinsics` gets a gradient from such a
    call only with pose_gradients (the depth term alone, which a call without either request sends it, is not formed next to it)."""
    s, v = extrinsics.shape[:2]
    ext = extrinsics.reshape(s * v, 4, 4)
    intr = intrinsics.reshape(s * v, 3, 3)
    nr, fr = near.reshape(s * v), far.reshape(s * v)
    _, _, _, n = gaussian_sh_coefficients.shape
    degree = isqrt(n) - 1
    # The depth channel: f(z) inside the kernels, always.  When the camera requires grad and the caller did not ask for the full
    # pose gradient, the reference's own graph still sends ONE gradient to it - through the depth render's extrinsics.inverse()
    # (cuda_splatting.py:239-242; training: model_wrapper.py:148-156 with config/main.yaml:50) - and the backward returns exactly
    # that term (GsrBackwardOptions.depth_term_only), carried to `extrinsics` by the closed-form backward of the camera set-up.
    fov = intrinsics_gradients and torch.is_grad_enabled() and intrinsics.requires_grad
    depth_cam = depth_mode is not None and not pose_gradients and not fov and _camera_wants_depth_gradient(extrinsics)
    viewbuf = _viewbuf(ext, intr, nr, fr, background_color.reshape(3), scale_invariant, pose_gradients or depth_cam, fov)
    channel = dict(extra_mode=depth_mode, camera_gradient="depth" if depth_cam else "full", return_alpha=alpha, intrinsics_gradients=fov)
    if gaussian_covariances is None:  # scale + quaternion records, as the encoder's adapter emits them
        records = _scale_rot_records(gaussian_scales, gaussian_rotations)
        color, depth, _, *acc = rasterize_views(
            gaussian_means, records, gaussian_opacities, gaussian_sh_coefficients, viewbuf, image_shape=image_shape,
            sh_degree=degree, use_sh=True, views_per_set=v, sh_planar=True, scale_rot=True, frames=frames, sh_frame=sh_frame, **channel)
    else:
        color, depth, _, *acc = rasterize_views(
            gaussian_means, gaussian_covariances, gaussian_opacities, gaussian_sh_coefficients, viewbuf,
            image_shape=image_shape, sh_degree=degree, use_sh=True, views_per_set=v, sh_planar=True, cov_3x3=True, sh_frame=sh_frame,
            **channel)
    h, w = image_shape
    color = color.reshape(s, v, 3, h, w)
    if depth is not None:
        depth = depth.reshape(s, v, h, w)
    if alpha:
        return color, depth, acc[0].reshape(s, v, h, w)
    return color, depth
