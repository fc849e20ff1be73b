"""Encoder-side Gaussian adapter: from per-pixel network outputs to the Gaussians the decoder renders - the step right in
front of the raster path.  Counterpart of the reference's `GaussianAdapter`
(src/model/encoder/common/gaussian_adapter.py:30-125; same constructor cfg, same `forward` arguments, `get_scale_multiplier`,
`d_sh`, `d_in`) with one difference in what comes out: the (N, 3, 3) world-space covariances are NOT materialised.  The
adapter returns scales, unit quaternions and the camera-to-world rotation of every source view; the raster library builds
Sigma = (C R) diag(s^2) (C R)^T in registers as it loads a Gaussian (`gsr_forward_ex`, `scale_rot`) and its backward returns
dL/dscale and dL/dquaternion directly.  That removes the 36 bytes per Gaussian the covariance costs in each direction (written
by the adapter, read by the forward, its gradient written by the backward and read by autograd) and six small torch
kernels.  `AdaptedGaussians.covariances` still yields the matrices (as differentiable torch ops) for callers that want them.

The harmonics are rotated into world space by `pf3plat_amd.sh_rotation.rotate_sh` (the reference uses its e3nn-based
src/misc/sh_rotation.py at gaussian_adapter.py:90); another callable of that signature, or None for no rotation, can be
passed to the constructor.  With `fuse_sh_rotation=True` they are not rotated at all: they stay in the source camera's frame
(`AdaptedGaussians.sh_frame` names the convention, `sh_basis`) and the raster kernels evaluate them at the view direction
carried into that frame (GSR_FLAG_SH_IN_FRAME) - the same image and gradients without the rotated copy and the per-Gaussian band
matrices torch's broadcasting builds.  `AdaptedGaussians.world_harmonics` still yields the rotated coefficients.

With `fused=True` the adapter's own arithmetic - K^-1, the ray, the mean, sigmoid and footprint of the scales, the quaternion
normalisation, the masked copy of the harmonics - is ONE HIP launch in each direction (`gsr_adapt` / `gsr_adapt_backward_ex`, an
autograd node of the compiled binding) instead of torch ops: `raw_gaussians` is read where it lies (the encoder's
`gaussians[..., 2:]` slice included), scales and rotations come back as the two slices of one (..., 7) record tensor - the form
the raster kernels take, which the decoder then passes on without a `cat` - and gradients reach raw_gaussians, depths,
coordinates, extrinsics and - when they require grad, as for any other input - intrinsics (through K^-1 of the ray and through
the footprint K[:2, :2]^-1 sets; the backward stays two launches).  It applies to calls whose per-Gaussian arguments all cover
the full (b, v, *rest) shape, in float32; any other call runs the torch ops below unchanged (`last_path` says which ran).  It is
independent of `fuse_sh_rotation`; PF3plat's training configuration is both.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from .sh_rotation import rotate_sh as _rotate_sh
from .types import Gaussians


@dataclass
class GaussianAdapterCfg:
    gaussian_scale_min: float
    gaussian_scale_max: float
    sh_degree: int


@dataclass
class AdaptedGaussians:
    """Per-pixel Gaussians of a batch of scenes, grouped by source view.  Every per-Gaussian tensor is (scene, view, *rest, ...),
    `rest` being whatever batch dimensions the encoder used behind the view axis (the reference calls the adapter with
    (ray, surface, sample), encoder_costvolume.py:529-540; a plain (ray,) works as well) - the shapes the reference's
    `Gaussians` has at that point, so `g.means[:, (0, -1)]`-style indexing reads the same."""

    means: Tensor  # (b, v, *rest, 3) world space
    scales: Tensor  # (b, v, *rest, 3)
    rotations: Tensor  # (b, v, *rest, 4) unit quaternions x, y, z, w, in the source camera's frame
    harmonics: Tensor  # (b, v, *rest, 3, d_sh)
    opacities: Tensor  # (b, v, *rest)
    frames: Tensor  # (b, v, 3, 3) camera-to-world rotation of every source view (no gradient)
    # None: `harmonics` are in world space; "e3nn" | "rasterizer": in the source camera's frame, to be rotated by `frames` in that
    # convention (GaussianAdapter(fuse_sh_rotation=True) - the raster kernels do it on the fly)
    sh_frame: Optional[str] = None

    @property
    def world_harmonics(self) -> Tensor:
        """(b, v, *rest, 3, d_sh) harmonics in world space, rotated with torch ops when they are in their frames (sh_frame): what the
        default adapter returns as `harmonics`, for callers that read the coefficients themselves (a .ply export, indexing)."""
        if self.sh_frame is None:
            return self.harmonics
        rest = self.opacities.dim() - 2
        return _rotate_sh(self.harmonics, self.frames[(slice(None), slice(None)) + (None,) * (rest + 1)], basis=self.sh_frame)

    @property
    def covariances(self) -> Tensor:
        """(b, v, *rest, 3, 3) world-space covariances, materialised with torch ops (the raster path does not need them)."""
        x, y, z, w = self.rotations.unbind(-1)
        t = 2 / ((self.rotations * self.rotations).sum(-1) + 1e-8)
        rot = torch.stack((1 - t * (y * y + z * z), t * (x * y - z * w), t * (x * z + y * w),
                           t * (x * y + z * w), 1 - t * (x * x + z * z), t * (y * z - x * w),
                           t * (x * z - y * w), t * (y * z + x * w), 1 - t * (x * x + y * y)), -1).unflatten(-1, (3, 3))
        rest = self.opacities.dim() - 2
        m = self.frames[(slice(None), slice(None)) + (None,) * rest] @ rot
        return (m * (self.scales * self.scales)[..., None, :]) @ m.transpose(-1, -2)

    def for_decoder(self, views: Optional[Sequence[int]] = None) -> Gaussians:
        """One set of Gaussians per scene in the decoder's layout: views flattened into the Gaussian axis (view-major, so the
        Gaussians of a source view are consecutive - the grouping the kernels' `frames` argument expects).  `views`: keep only
        these source views (the reference keeps the first and the last, `[:, (0, -1)]`, encoder_costvolume.py:556-573)."""
        pick = (lambda t: t) if views is None else (lambda t: t[:, list(views)])
        b = self.opacities.shape[0]
        flat = lambda t, k: pick(t).reshape(b, -1, *t.shape[t.dim() - k:])
        return Gaussians(means=flat(self.means, 1), covariances=None, harmonics=flat(self.harmonics, 2),
                         opacities=flat(self.opacities, 0), scales=flat(self.scales, 1), rotations=flat(self.rotations, 1),
                         frames=pick(self.frames), sh_frame=self.sh_frame)


class GaussianAdapter(nn.Module):
    """fuse_sh_rotation: leave the harmonics in the source camera's frame and let the raster kernels rotate the view direction
    instead (module docstring); `sh_basis` is then the convention ("e3nn", the reference's, or "rasterizer") and `rotate_sh` is
    not used.  fused: run the adapter's arithmetic as one HIP launch each way where the call's shapes allow it (module docstring)."""

    def __init__(self, cfg: GaussianAdapterCfg, rotate_sh: Optional[Callable[[Tensor, Tensor], Tensor]] = _rotate_sh,
                 fuse_sh_rotation: bool = False, sh_basis: str = "e3nn", fused: bool = False):
        super().__init__()
        if sh_basis not in ("e3nn", "rasterizer"):
            raise ValueError(f"sh_basis must be 'e3nn' or 'rasterizer', got {sh_basis!r}")
        self.cfg = cfg
        self.rotate_sh = rotate_sh
        self.fuse_sh_rotation = fuse_sh_rotation
        self.sh_basis = sh_basis
        self.fused = fused
        self._last_path: Optional[str] = None
        # band l of the harmonics starts small (0.1 x 0.25^l): the DC term dominates at initialisation
        band = torch.arange(self.d_sh, dtype=torch.float32).sqrt().floor()
        self.register_buffer("sh_mask", torch.where(band == 0, torch.ones(()), 0.1 * 0.25 ** band), persistent=False)

    @property
    def d_sh(self) -> int:
        return (self.cfg.sh_degree + 1) ** 2

    @property
    def d_in(self) -> int:
        return 7 + 3 * self.d_sh

    @property
    def last_path(self) -> Optional[str]:
        """Which path the last `forward` took: "hip" (the compiled launch) or "torch" (the torch ops); None before the first call."""
        return self._last_path

    def _hip_applies(self, extrinsics: Tensor, intrinsics: Tensor, coordinates: Tensor, depths: Tensor, raw_gaussians: Tensor, full: tuple) -> bool:
        """The compiled path covers calls whose per-Gaussian arguments all have the full (b, v, *rest) shape (every shipped config:
        one surface, one Gaussian per pixel) and one camera per view, in float32.  Whether the intrinsics require grad does not matter:
        their gradient comes out of the same backward launches."""
        if not self.fused or self.cfg.sh_degree > 4:
            return False
        if tuple(depths.shape) != full or tuple(coordinates.shape) != (*full, 2) or tuple(raw_gaussians.shape) != (*full, self.d_in):
            return False
        if tuple(intrinsics.shape[:2]) != full[:2] or any(d != 1 for d in intrinsics.shape[2:-2]) or tuple(intrinsics.shape[-2:]) != (3, 3):
            return False
        return all(t.dtype == torch.float32 for t in (extrinsics, intrinsics, coordinates, depths, raw_gaussians))

    def get_scale_multiplier(self, intrinsics: Tensor, pixel_size: Tensor, multiplier: float = 0.1) -> Tensor:
        """How large one pixel is at unit depth, summed over x and y: (K[:2, :2]^-1 pixel_size) . (1, 1), times `multiplier`."""
        return multiplier * torch.linalg.solve(intrinsics[..., :2, :2], pixel_size.expand(*intrinsics.shape[:-2], 2)).sum(-1)

    def forward(self, extrinsics: Tensor, intrinsics: Tensor, coordinates: Tensor, depths: Tensor, opacities: Tensor,
                raw_gaussians: Tensor, image_shape: tuple, eps: float = 1e-8) -> AdaptedGaussians:
        """The reference's `*#batch` call shapes (gaussian_adapter.py:48-58): every argument broadcasts against
        `opacities.shape` = (b, v, *rest).  extrinsics (b, v, 1.., 4, 4) / intrinsics (b, v, 1.., 3, 3) of the source views (one
        camera per view: singleton dims behind the view axis), coordinates (b, v, *rest#, 2) in [0, 1]^2, depths (b, v, *rest#),
        raw_gaussians (b, v, *rest#, 7 + 3 d_sh) = scale(3) | quaternion xyzw(4) | harmonics(3 x d_sh).  E.g. the encoder's call
        (encoder_costvolume.py:529-540): extrinsics (b, v, 1, 1, 1, 4, 4), coordinates (b, v, r, srf, 1, 2), depths (b, v, r, 1, 1),
        opacities (b, v, r, srf, spp), raw (b, v, r, srf, 1, c)."""
        h, w = image_shape
        full = tuple(opacities.shape)  # (b, v, *rest)
        if len(full) < 3:
            raise ValueError(f"opacities must be (scene, view, ray, ...), got {full}")
        if any(d != 1 for d in extrinsics.shape[2:-2]) or tuple(extrinsics.shape[:2]) != full[:2]:
            raise ValueError("one camera per (scene, view): extrinsics must be (b, v, 1.., 4, 4); a rotation per Gaussian cannot be "
                             "expressed as the per-view frames the raster kernels take")
        lo, hi = self.cfg.gaussian_scale_min, self.cfg.gaussian_scale_max
        c2w = extrinsics[..., :3, :3].detach()
        if self._hip_applies(extrinsics, intrinsics, coordinates, depths, raw_gaussians, full):
            from . import _lib

            groups = full[0] * full[1]
            means, records, harmonics = _lib.load_torch_ext().adapt(
                extrinsics.reshape(groups, 4, 4), intrinsics.reshape(groups, 3, 3), coordinates.reshape(groups, -1, 2), depths.reshape(groups, -1),
                raw_gaussians, float(lo), float(hi), int(h), int(w), float(eps), int(self.cfg.sh_degree))
            self._last_path = "hip"
            means, records, harmonics = means.view(*full, 3), records.view(*full, 7), harmonics.view(*full, 3, self.d_sh)
            scales, rotations = records[..., :3], records[..., 3:]  # two slices of ONE record tensor: the decoder passes it on as it is
        else:
            self._last_path = "torch"
            means, scales, rotations, harmonics = self._torch_forward(extrinsics, intrinsics, coordinates, depths, raw_gaussians, full, h, w, eps)
        sh_frame = None
        if self.fuse_sh_rotation:
            # rotate_sh's rule (reference sh_rotation.py:20-21): no rotation at all unless every frame is proper - then the
            # harmonics are left as they are and count as world space (sh_frame None), exactly what the torch rotation returns
            if torch.allclose(torch.det(c2w), c2w.new_tensor(1)):
                sh_frame = self.sh_basis
        elif self.rotate_sh is not None:
            harmonics = self.rotate_sh(harmonics, c2w[..., None, :, :])
        return AdaptedGaussians(means=means, scales=scales, rotations=rotations, harmonics=harmonics, opacities=opacities,
                                frames=c2w.reshape(*full[:2], 3, 3), sh_frame=sh_frame)

    def _torch_forward(self, extrinsics: Tensor, intrinsics: Tensor, coordinates: Tensor, depths: Tensor, raw_gaussians: Tensor, full: tuple,
                       h: int, w: int, eps: float):
        """The adapter's arithmetic as torch ops -> means, scales, rotations (each broadcast to `full`) and masked, un-rotated harmonics."""
        lo, hi = self.cfg.gaussian_scale_min, self.cfg.gaussian_scale_max
        raw_scale, raw_quat, raw_sh = raw_gaussians.split((3, 4, 3 * self.d_sh), dim=-1)
        pixel = torch.tensor((1.0 / w, 1.0 / h), dtype=intrinsics.dtype, device=extrinsics.device)
        footprint = depths * self.get_scale_multiplier(intrinsics, pixel)  # world size of 0.1 pixel at the Gaussian's depth
        scales = (lo + (hi - lo) * raw_scale.sigmoid()) * footprint[..., None]
        rotations = raw_quat / (raw_quat.norm(dim=-1, keepdim=True) + eps)
        harmonics = raw_sh.unflatten(-1, (3, self.d_sh)).broadcast_to((*full, 3, self.d_sh)) * self.sh_mask
        # mean = camera centre + depth x (unit ray through the pixel, rotated into world space)
        ray = torch.linalg.solve(intrinsics, F.pad(coordinates, (0, 1), value=1.0).unsqueeze(-1)).squeeze(-1)
        ray = F.normalize(ray, dim=-1)
        direction = (extrinsics[..., :3, :3] @ ray.unsqueeze(-1)).squeeze(-1)
        means = extrinsics[..., :3, 3] + direction * depths[..., None]
        return means.broadcast_to((*full, 3)), scales.broadcast_to((*full, 3)), rotations.broadcast_to((*full, 4)), harmonics
