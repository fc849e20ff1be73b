"""Keypoint extraction on the device: what SuperPoint.forward does after its last two convolutions - the 65-way softmax, the 8 x 8
depth-to-space, simple_nms, the border cut, torch.where against the threshold, the dense descriptor normalisation and
sample_descriptors (reference src/model/LightGlue/lightglue/superpoint.py:52-95, 171-227, with the rescale of utils.py:146; the
definition is stated in include/gsr.h).  `detect_keypoints` runs a whole batch of images in one chain of up to six launches
(gsr_keypoints): the score map is the one dense array, NMS works on tiles of TILE x TILE pixels in LDS, the compaction is ordered, the
normalised descriptor map is never formed, and nothing is read back until the caller asks for the lengths - `Keypoints.lengths()`,
one read of the counts for the whole batch.  Forward only, as the reference runs the extractor under no_grad.  There is no CPU
fallback.  SuperPoint's convolutions stay torch."""
from __future__ import annotations

import ctypes
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from ._call import f32, launch, ptr, require_device, scratch

TILE = 32          # the NMS tile's edge in pixels (gsr_keypoints_tile()): a tile row is one word of the keep mask
MAX_CHANNELS = 256
MAX_RADIUS = 4
FROM_LOGITS, FROM_SCORES = 0, 1


class PackedKeypoints(NamedTuple):
    keypoints: Tensor              # (sum n_b, 2) float32 (x, y), image after image
    pixels: Tensor                 # (sum n_b, 2) int32 (x, y)
    keypoint_scores: Tensor        # (sum n_b,)
    descriptors: Optional[Tensor]  # (sum n_b, C)
    lengths: Tuple[int, ...]       # n_b


class Keypoints(NamedTuple):
    keypoints: Tensor              # (B capacity, 2) float32 (x, y): image b's rows follow those of the images before it, no gaps
    pixels: Tensor                 # (B capacity, 2) int32 (x, y), before the rescale
    keypoint_scores: Tensor        # (B capacity,) float32
    descriptors: Optional[Tensor]  # (B capacity, C) float32, L2-normalised
    counts: Tensor                 # (B,) int32, on the device: the number FOUND per image, whatever the capacity
    capacity: int
    size: Tuple[int, int]          # (H, W)
    max_num_keypoints: Optional[int] = None

    def lengths(self) -> Tuple[int, ...]:
        """The rows per image: the one host read of the batch.  Raises if an image found more keypoints than `capacity` rows."""
        counts = self.counts.tolist()
        for b, c in enumerate(counts):
            if c > self.capacity:
                raise RuntimeError(f"detect_keypoints: image {b} has {c} keypoints, capacity is {self.capacity} rows per image: "
                                   "call again with capacity >= that count (nothing was written past the capacity)")
        k = self.max_num_keypoints
        return tuple(c if k is None else min(c, k) for c in counts)

    def packed(self) -> PackedKeypoints:
        """The arrays sliced to the total, and the lengths: `keypoints` and `lengths` are what `match_assignment`'s ragged form takes
        as kpts0 / kpts1 and lengths0 / lengths1."""
        lengths = self.lengths()
        n = sum(lengths)
        return PackedKeypoints(self.keypoints[:n], self.pixels[:n], self.keypoint_scores[:n],
                               None if self.descriptors is None else self.descriptors[:n], lengths)

    def lists(self) -> List[Dict[str, Optional[Tensor]]]:
        """Per image the reference's `keypoints` (n, 2), `keypoint_scores` (n,) and `descriptors` (n, C).  One host read, then slices."""
        p, out, o = self.packed(), [], 0
        for n in p.lengths:
            out.append({"keypoints": p.keypoints[o:o + n], "keypoint_scores": p.keypoint_scores[o:o + n],
                        "descriptors": None if p.descriptors is None else p.descriptors[o:o + n], "pixels": p.pixels[o:o + n]})
            o += n
        return out


def _check(name, B, H, W, descriptors, hw, scales, nms_radius, detection_threshold, remove_borders, max_num_keypoints, capacity):
    """The shape and range checks of either form: before the device is looked at and before the library is loaded."""
    C = 0
    if descriptors is not None:
        if descriptors.dim() != 4 or descriptors.shape[0] != B:
            raise ValueError(f"{name}: expected descriptors ({B}, C, h, w), got {tuple(descriptors.shape)}")
        C = descriptors.shape[1]
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"{name}: supports 1 <= C <= {MAX_CHANNELS} descriptor channels, got {C}")
        if hw is None and (H % 8 or W % 8):
            raise ValueError(f"{name}: with descriptors H and W must be multiples of 8, got {H} x {W}")
        if tuple(descriptors.shape[2:]) != (H // 8, W // 8):
            raise ValueError(f"{name}: descriptors are {tuple(descriptors.shape[2:])} cells, the scores {H // 8} x {W // 8}")
    if scales is not None and tuple(scales.shape) != (B, 2):
        raise ValueError(f"{name}: expected scales ({B}, 2), got {tuple(scales.shape)}")
    if int(nms_radius) != nms_radius or not 0 <= nms_radius <= MAX_RADIUS:
        raise ValueError(f"{name}: supports 0 <= nms_radius <= {MAX_RADIUS}, got {nms_radius!r}")
    if int(remove_borders) != remove_borders or remove_borders < 0:
        raise ValueError(f"{name}: remove_borders must be an int >= 0, got {remove_borders!r}")
    if int(capacity) != capacity or capacity < 1:
        raise ValueError(f"{name}: capacity must be an int >= 1 (rows per image), got {capacity!r}")
    if max_num_keypoints is not None and (int(max_num_keypoints) != max_num_keypoints or max_num_keypoints < 1):
        raise ValueError(f"{name}: max_num_keypoints must be None or an int >= 1, got {max_num_keypoints!r}")
    t = float(detection_threshold)
    if t != t or t < 0 or t == float("inf"):
        raise ValueError(f"{name}: detection_threshold must be finite and >= 0, got {detection_threshold!r}")
    if not 1 <= B <= 65535:
        raise ValueError(f"{name}: supports 1 <= B <= 65535 images, got {B}")
    if B * H * W > 0x7fffffff or B * int(capacity) * max(C, 2) > 0x7fffffff:
        raise ValueError(f"{name}: more than 2^31 - 1 elements in an array")
    return C


def _run(mode, logits, scores, descriptors, scales, B, H, W, C, nms_radius, detection_threshold, remove_borders, max_num_keypoints, capacity):
    dev, cap = scores.device, int(capacity)
    desc = strides = None
    if descriptors is not None:  # read where it lies, through its strides: contiguous and channels_last alike
        desc = descriptors.detach()
        desc = desc if desc.dtype == torch.float32 else desc.to(torch.float32)
        strides = (ctypes.c_int64 * 4)(*desc.stride())
    sc = None if scales is None else f32(scales)
    kpts = torch.empty(B * cap, 2, dtype=torch.float32, device=dev)   # (written up to the batch's total)
    pixels = torch.empty(B * cap, 2, dtype=torch.int32, device=dev)
    kscores = torch.empty(B * cap, dtype=torch.float32, device=dev)
    out_desc = torch.empty(B * cap, C, dtype=torch.float32, device=dev) if C else None
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    work = scratch(_lib.load().gsr_keypoints_scratch_bytes(B, H, W, C, cap), torch.int32, dev)
    launch("gsr_keypoints", dev, mode, B, H, W, C, int(nms_radius), float(detection_threshold), int(remove_borders),
           int(max_num_keypoints or 0), cap, ptr(logits), scores.data_ptr(), ptr(desc), strides, ptr(sc), work.data_ptr(), kpts.data_ptr(),
           pixels.data_ptr(), kscores.data_ptr(), ptr(out_desc), counts.data_ptr())
    return Keypoints(kpts, pixels, kscores, out_desc, counts, cap, (H, W), None if max_num_keypoints is None else int(max_num_keypoints))


@torch.no_grad()
def detect_keypoints(logits: Tensor, descriptors: Tensor, scales: Optional[Tensor] = None, *, nms_radius: int = 4,
                     detection_threshold: float = 0.0005, remove_borders: int = 4, max_num_keypoints: Optional[int] = None,
                     capacity: int = 4096) -> Keypoints:
    """convPb's output `logits` (B, 65, h, w), before the softmax, and convDb's output `descriptors` (B, C, h, w), 1 <= C <= 256, not
    normalised (contiguous or channels_last: read through its strides) -> Keypoints of the B images of 8 h x 8 w pixels, as
    include/gsr.h defines them: SuperPoint.forward's lines after the convolutions.  `scales` (B, 2): the preprocessor's (sx, sy);
    keypoints are (pixel + 0.5) / scale - 0.5.  `max_num_keypoints` = k: an image with more keeps its k highest scores in descending
    order, ties to the lower row-major index.  `capacity`: rows per image; an image that finds more overflows - `lengths()` raises,
    naming the count.  Up to six launches, no host synchronisation, the same bits on every call."""
    if logits.dim() != 4 or logits.shape[1] != 65:
        raise ValueError(f"detect_keypoints: expected logits (B, 65, h, w), got {tuple(logits.shape)}")
    if descriptors is None:
        raise ValueError("detect_keypoints: needs the descriptors (keypoints_from_scores runs without)")
    B, _, h, w = logits.shape
    if h < 1 or w < 1:
        raise ValueError(f"detect_keypoints: needs at least one cell, got {h} x {w}")
    C = _check("detect_keypoints", B, 8 * h, 8 * w, descriptors, (h, w), scales, nms_radius, detection_threshold, remove_borders,
               max_num_keypoints, capacity)
    require_device("keypoints", "detect_keypoints", [logits, descriptors] + ([scales] if scales is not None else []))
    lg = f32(logits)
    scores = torch.empty(B, 8 * h, 8 * w, dtype=torch.float32, device=lg.device)  # (the one dense array: fully written by the call)
    return _run(FROM_LOGITS, lg, scores, descriptors, scales, B, 8 * h, 8 * w, C, nms_radius, detection_threshold, remove_borders,
                max_num_keypoints, capacity)


@torch.no_grad()
def keypoints_from_scores(scores: Tensor, descriptors: Optional[Tensor] = None, scales: Optional[Tensor] = None, *, nms_radius: int = 4,
                          detection_threshold: float = 0.0005, remove_borders: int = 4, max_num_keypoints: Optional[int] = None,
                          capacity: int = 4096) -> Keypoints:
    """The same chain entered after the softmax: `scores` (B, H, W), for callers with another detector.  From here on every decision
    is a comparison, so the result is exact.  H and W need not be multiples of 8 when `descriptors` is None."""
    if scores.dim() != 3 or scores.shape[1] < 1 or scores.shape[2] < 1:
        raise ValueError(f"keypoints_from_scores: expected scores (B, H, W), got {tuple(scores.shape)}")
    B, H, W = scores.shape
    C = _check("keypoints_from_scores", B, H, W, descriptors, None, scales, nms_radius, detection_threshold, remove_borders,
               max_num_keypoints, capacity)
    require_device("keypoints", "keypoints_from_scores", [scores] + [t for t in (descriptors, scales) if t is not None])
    return _run(FROM_SCORES, None, f32(scores), descriptors, scales, B, H, W, C, nms_radius, detection_threshold, remove_borders,
                max_num_keypoints, capacity)


class SuperPoint(nn.Module):
    """SuperPoint (superpoint.py:98-227) with the reference's parameter names (conv1a ... convDb: its state dict loads with
    strict=True).  The constructor downloads nothing: load the weights with `load_state_dict`.  `forward({"image": (B, 1 or 3, H, W)})`
    takes a batch of equally sized images (H and W multiples of 8), turns RGB to grey with the weights 0.299, 0.587, 0.114, runs the
    convolutions in torch and `detect_keypoints` on the two heads' outputs, and returns `Keypoints`.  The preprocessor's resize stays
    with the caller, who passes its `scales` (B, 2) in the dict."""

    def __init__(self, descriptor_dim: int = 256, nms_radius: int = 4, max_num_keypoints: Optional[int] = None,
                 detection_threshold: float = 0.0005, remove_borders: int = 4, capacity: int = 4096) -> None:
        super().__init__()
        if not 1 <= descriptor_dim <= MAX_CHANNELS:
            raise ValueError(f"SuperPoint: the device head supports 1 <= descriptor_dim <= {MAX_CHANNELS}, got {descriptor_dim}")
        if max_num_keypoints is not None and max_num_keypoints <= 0:
            raise ValueError("max_num_keypoints must be positive or None")
        self.conf = dict(nms_radius=nms_radius, max_num_keypoints=max_num_keypoints, detection_threshold=detection_threshold,
                         remove_borders=remove_borders, capacity=capacity)
        self.relu = nn.ReLU(inplace=True)
        self.pool = nn.MaxPool2d(kernel_size=2, stride=2)
        c1, c2, c3, c4, c5 = 64, 64, 128, 128, 256
        conv = lambda i, o, k: nn.Conv2d(i, o, kernel_size=k, stride=1, padding=k // 2)
        self.conv1a, self.conv1b = conv(1, c1, 3), conv(c1, c1, 3)
        self.conv2a, self.conv2b = conv(c1, c2, 3), conv(c2, c2, 3)
        self.conv3a, self.conv3b = conv(c2, c3, 3), conv(c3, c3, 3)
        self.conv4a, self.conv4b = conv(c3, c4, 3), conv(c4, c4, 3)
        self.convPa, self.convPb = conv(c4, c5, 3), conv(c5, 65, 1)
        self.convDa, self.convDb = conv(c4, c5, 3), conv(c5, descriptor_dim, 1)

    @torch.no_grad()
    def heads(self, image: Tensor) -> Tuple[Tensor, Tensor]:
        """The torch part: image (B, 1 or 3, H, W) -> convPb's logits (B, 65, H / 8, W / 8) and convDb's descriptors."""
        if image.dim() != 4 or image.shape[1] not in (1, 3) or image.shape[2] % 8 or image.shape[3] % 8:
            raise ValueError(f"SuperPoint: expected images (B, 1 or 3, H, W) with H and W multiples of 8, got {tuple(image.shape)}")
        if image.shape[1] == 3:
            image = (image * image.new_tensor([0.299, 0.587, 0.114]).view(1, 3, 1, 1)).sum(1, keepdim=True)
        x = self.relu(self.conv1a(image))
        x = self.pool(self.relu(self.conv1b(x)))
        x = self.relu(self.conv2a(x))
        x = self.pool(self.relu(self.conv2b(x)))
        x = self.relu(self.conv3a(x))
        x = self.pool(self.relu(self.conv3b(x)))
        x = self.relu(self.conv4a(x))
        x = self.relu(self.conv4b(x))
        return self.convPb(self.relu(self.convPa(x))), self.convDb(self.relu(self.convDa(x)))

    def forward(self, data: dict) -> Keypoints:
        logits, descriptors = self.heads(data["image"])
        return detect_keypoints(logits, descriptors, data.get("scales"), **self.conf)
