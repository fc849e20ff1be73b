"""The tail of the matcher on the device: LightGlue's MatchAssignment after its projections, sigmoid_log_double_softmax, filter_matches
and the list building (reference src/model/LightGlue/lightglue/lightglue.py:259-312, 586-597; the definition is stated in
include/gsr.h).  `match_assignment` runs every (pair, scene) list of a batch in one chain of three launches (gsr_match_assignment):
the similarity is formed 32 x 32 at a time and dropped, no array of m x n elements exists, and nothing is read back until the caller
asks for the packed lists - `Matches.lists()` or `pack_matched`, one read of the counts for the whole batch.  Forward only, as the
reference runs the matcher under no_grad.  There is no CPU fallback.  The two projections stay torch."""
from __future__ import annotations

import ctypes
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from ._call import f32, launch, ptr, require_device, scratch
from .losses import PackedCorrespondences

MAX_DIM = 256


class Matches(NamedTuple):
    matches0: Tensor          # int64, -1 where none: (B, m) in the equal-length form, (sum m_l,) packed; indices local to the list
    matches1: Tensor          # (B, n) or (sum n_l,)
    matching_scores0: Tensor  # float32, 0 where the keypoint has no mutual partner
    matching_scores1: Tensor
    idx0: Tensor              # (sum m_l,) int32: list l's valid rows in ascending order at entries offsets0[l] .. + counts[l]
    idx1: Tensor              # (sum m_l,) int32: their partners
    scores: Tensor            # (sum m_l,) float32
    counts: Tensor            # (L,) int32, on the device
    offsets0: tuple           # L + 1 Python ints
    offsets1: tuple
    ids_i: Optional[Tensor] = None      # (sum m_l,) int64 flat pixel y * width + x of the compact entries, with keypoints
    ids_j: Optional[Tensor] = None
    points_2d: Optional[Tensor] = None  # (sum m_l, 2) the first image's sub-pixel (x, y) of the compact entries

    def _entries(self) -> Tuple[List[int], Tensor]:
        """The one host read - the counts of the whole call - and the positions of the valid compact entries, list after list."""
        counts = self.counts.tolist()
        dev = self.idx0.device
        if sum(counts) == 0:
            return counts, torch.empty(0, dtype=torch.int64, device=dev)
        return counts, torch.cat([torch.arange(o, o + c, device=dev) for o, c in zip(self.offsets0, counts)])

    def lists(self):
        """[(matches (k, 2) int64, scores (k,)) per list]: the reference's `matches` and `scores` (lightglue.py:588-597).  One host
        read of `counts` for the whole call, then slices."""
        counts = self.counts.tolist()
        out = []
        for o, c in zip(self.offsets0, counts):
            out.append((torch.stack([self.idx0[o:o + c], self.idx1[o:o + c]], -1).to(torch.int64), self.scores[o:o + c]))
        return out


def _offsets(lengths, name: str) -> tuple:
    out = [0]
    for n in lengths:
        if int(n) != n or n < 0:
            raise ValueError(f"match_assignment: {name} holds list lengths, Python ints >= 0, got {n!r}")
        out.append(out[-1] + int(n))
    return tuple(out)


def _assignment_args(mdesc0, mdesc1, z0, z1, lengths0, lengths1, threshold, scale, kpts0, kpts1, width):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if (lengths0 is None) != (lengths1 is None):
        raise ValueError("match_assignment: lengths0 and lengths1 go together")
    if lengths0 is None:
        if mdesc0.dim() != 3 or mdesc1.dim() != 3 or mdesc0.shape[0] != mdesc1.shape[0] or mdesc0.shape[2] != mdesc1.shape[2]:
            raise ValueError(f"match_assignment: expected mdesc0 (B, m, d) and mdesc1 (B, n, d), got {tuple(mdesc0.shape)}, {tuple(mdesc1.shape)}")
        B, m, d = mdesc0.shape
        n = mdesc1.shape[1]
        if B < 1:
            raise ValueError("match_assignment: needs at least one list")
        for name, z, k in (("z0", z0, m), ("z1", z1, n)):
            if tuple(z.shape) not in ((B, k), (B, k, 1)):
                raise ValueError(f"match_assignment: expected {name} ({B}, {k}) or ({B}, {k}, 1), got {tuple(z.shape)}")
        off0, off1, batch = tuple(range(0, B * m + 1, m)) if m else (0,) * (B + 1), tuple(range(0, B * n + 1, n)) if n else (0,) * (B + 1), (B, m, n)
    else:
        off0, off1, batch = _offsets(lengths0, "lengths0"), _offsets(lengths1, "lengths1"), None
        if len(off0) != len(off1) or len(off0) < 2:
            raise ValueError(f"match_assignment: needs as many lengths0 as lengths1 and at least one list, got {len(off0) - 1} and {len(off1) - 1}")
        if mdesc0.dim() != 2 or mdesc1.dim() != 2 or mdesc0.shape[1] != mdesc1.shape[1]:
            raise ValueError(f"match_assignment: expected packed mdesc0 (sum m, d) and mdesc1 (sum n, d), got {tuple(mdesc0.shape)}, {tuple(mdesc1.shape)}")
        d = mdesc0.shape[1]
        for name, t, total in (("mdesc0", mdesc0, off0[-1]), ("mdesc1", mdesc1, off1[-1])):
            if t.shape[0] != total:
                raise ValueError(f"match_assignment: {name} has {t.shape[0]} rows, the lengths sum to {total}")
        for name, z, k in (("z0", z0, off0[-1]), ("z1", z1, off1[-1])):
            if tuple(z.shape) not in ((k,), (k, 1)):
                raise ValueError(f"match_assignment: expected {name} ({k},) or ({k}, 1), got {tuple(z.shape)}")
    if not 1 <= d <= MAX_DIM:
        raise ValueError(f"match_assignment: supports 1 <= d <= {MAX_DIM} channels, got {d}")
    if max(off0[-1], off1[-1]) * d > 0x7fffffff:
        raise ValueError("match_assignment: more than 2^31 - 1 elements in an array")
    scale = d ** -0.5 if scale is None else float(scale)
    threshold = float(threshold)
    for name, x in (("scale", scale), ("threshold", threshold)):
        if x != x or x in (float("inf"), float("-inf")):
            raise ValueError(f"match_assignment: {name} must be finite, got {x}")
    if (kpts0 is None) != (kpts1 is None):
        raise ValueError("match_assignment: kpts0 and kpts1 go together")
    if kpts0 is not None:
        if width is None or int(width) < 1:
            raise ValueError(f"match_assignment: keypoints need the image width, a positive int, got {width!r}")
        for name, t, total in (("kpts0", kpts0, off0[-1]), ("kpts1", kpts1, off1[-1])):
            if t.shape[-1:] != (2,) or t.numel() != 2 * total or t.dim() != (2 if batch is None else 3):
                raise ValueError(f"match_assignment: expected {name} with {total} keypoints (x, y), got {tuple(t.shape)}")
    tensors = [mdesc0, mdesc1, z0, z1] + ([kpts0, kpts1] if kpts0 is not None else [])
    require_device("matching", "match_assignment", tensors)
    return off0, off1, d, scale, threshold, batch


@torch.no_grad()
def match_assignment(mdesc0: Tensor, mdesc1: Tensor, z0: Tensor, z1: Tensor, lengths0: Optional[Sequence[int]] = None,
                     lengths1: Optional[Sequence[int]] = None, threshold: float = 0.1, scale: Optional[float] = None,
                     kpts0: Optional[Tensor] = None, kpts1: Optional[Tensor] = None, width: Optional[int] = None) -> Matches:
    """The outputs of final_proj (NOT divided by d ** 0.25) and the matchability logits -> Matches, as include/gsr.h defines it: the
    reference's `filter_matches(sigmoid_log_double_softmax(sim, z0, z1), threshold)` and its per-list `matches` / `scores`, without the
    similarity, the log assignment matrix or a `torch.where`.  Either the reference's equal-length form - mdesc0 (B, m, d), mdesc1
    (B, n, d), z0 (B, m[, 1]), z1 (B, n[, 1]): B lists - or the packed ragged form - (sum m_l, d), (sum n_l, d), (sum m_l[, 1]),
    (sum n_l[, 1]) with `lengths0` / `lengths1`, the lists' sizes as Python ints.  1 <= d <= 256; `scale` defaults to d ** -0.5 and
    multiplies the similarity.  Ties go to the lowest index; a list with an empty side has no matches.  `kpts0` / `kpts1` (x, y) in the
    operands' form and the image `width`: the compact entries also carry ids_i, ids_j (trunc(y) * width + trunc(x), int64) and the
    first image's sub-pixel points_2d.  Three launches, no host synchronisation, the same bits on every call."""
    off0, off1, d, scale, threshold, batch = _assignment_args(mdesc0, mdesc1, z0, z1, lengths0, lengths1, threshold, scale, kpts0, kpts1, width)
    dev, L, M0, M1 = mdesc0.device, len(off0) - 1, off0[-1], off1[-1]
    a0, a1, b0, b1 = f32(mdesc0), f32(mdesc1), f32(z0), f32(z1)
    k0, k1 = (f32(kpts0), f32(kpts1)) if kpts0 is not None else (None, None)
    host0, host1 = (ctypes.c_int32 * (L + 1))(*off0), (ctypes.c_int32 * (L + 1))(*off1)
    both = torch.tensor([off0, off1], dtype=torch.int32)
    both = both.pin_memory().to(dev, non_blocking=True)  # (from the shapes: goes up without waiting)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    fl = lambda *n: torch.empty(n, dtype=torch.float32, device=dev)
    matches0, matches1, mscores0, mscores1 = i32(M0), i32(M1), fl(M0), fl(M1)  # (fully written by the call)
    idx0, idx1, score, counts = i32(M0), i32(M0), fl(M0), i32(L)               # (written up to each list's count)
    ids_i = ids_j = points = None
    if k0 is not None:
        ids_i, ids_j = (torch.empty(M0, dtype=torch.int64, device=dev) for _ in range(2))
        points = fl(M0, 2)
    work = scratch(_lib.load().gsr_match_assignment_scratch_bytes(L, host0, host1, d), torch.float32, dev)
    launch("gsr_match_assignment", dev, L, d, scale, threshold, int(width) if k0 is not None else 0, a0.data_ptr(), a1.data_ptr(),
           b0.data_ptr(), b1.data_ptr(), host0, both[0].data_ptr(), host1, both[1].data_ptr(), ptr(k0), ptr(k1), work.data_ptr(),
           matches0.data_ptr(), matches1.data_ptr(), mscores0.data_ptr(), mscores1.data_ptr(), idx0.data_ptr(), idx1.data_ptr(),
           score.data_ptr(), ptr(ids_i), ptr(ids_j), ptr(points), counts.data_ptr())
    dense = [matches0.to(torch.int64), matches1.to(torch.int64), mscores0, mscores1]
    if batch is not None:
        B, m, n = batch
        dense = [t.reshape(B, k) for t, k in zip(dense, (m, n, m, n))]
    return Matches(*dense, idx0, idx1, score, counts, off0, off1, ids_i, ids_j, points)


def pack_matched(matches: Matches, num_scenes: int) -> Tuple[PackedCorrespondences, Tensor]:
    """Matches of a call made with keypoints, list l = pair x num_scenes + scene -> (PackedCorrespondences, points_2d (M, 2)): what
    `pose.coarse_poses(xyz, intrinsics_px, packed, points_2d=points_2d)` reads, `conf` zeros as `pose.pack_matches` leaves it.  The
    one host read of the counts, then one gather per array.  Raises unless the list count is num_scenes times v (v - 1) / 2 pairs."""
    L, b = len(matches.offsets0) - 1, int(num_scenes)
    pairs = L // b if b >= 1 and L % b == 0 else 0
    v = 2
    while v * (v - 1) // 2 < pairs:
        v += 1
    if pairs < 1 or v * (v - 1) // 2 != pairs:
        raise ValueError(f"pack_matched: {L} lists are not {num_scenes} scenes times the v (v - 1) / 2 pairs of v views")
    if matches.ids_i is None:
        raise ValueError("pack_matched: the matches carry no pixel ids: call match_assignment with kpts0, kpts1 and width")
    counts, where = matches._entries()
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + c)
    dev = matches.idx0.device
    off = torch.tensor(offsets, dtype=torch.int32)
    off = off.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else off
    conf = torch.zeros(L, dtype=torch.float32, device=dev)
    packed = PackedCorrespondences(matches.ids_i[where], matches.ids_j[where], matches.scores[where], conf, tuple(offsets), off, b, pairs)
    return packed, matches.points_2d[where]


class MatchAssignment(nn.Module):
    """LightGlue's MatchAssignment (lightglue.py:274-293) with the reference's parameter names (matchability, final_proj: its state
    dict loads with strict=True).  `forward` runs the two nn.Linear in torch and `match_assignment` on their outputs, and returns
    `Matches` - what the reference's `filter_matches(scores, filter_threshold)` makes of this module's output, lists included.  The
    reference's forward returns the log assignment matrix (and the similarity): exactly the (m + 1) x (n + 1) array that is NOT
    formed here."""

    def __init__(self, dim: int) -> None:
        super().__init__()
        if not 1 <= dim <= MAX_DIM:
            raise ValueError(f"MatchAssignment: the device assignment supports 1 <= dim <= {MAX_DIM}, got {dim}")
        self.dim = dim
        self.matchability = nn.Linear(dim, 1, bias=True)
        self.final_proj = nn.Linear(dim, dim, bias=True)

    def forward(self, desc0: Tensor, desc1: Tensor, filter_threshold: float = 0.1, kpts0: Optional[Tensor] = None,
                kpts1: Optional[Tensor] = None, width: Optional[int] = None) -> Matches:
        """desc0 (B, m, dim), desc1 (B, n, dim) -> Matches of B lists."""
        with torch.no_grad():
            mdesc0, mdesc1 = self.final_proj(desc0), self.final_proj(desc1)
            z0, z1 = self.matchability(desc0), self.matchability(desc1)
        return match_assignment(mdesc0, mdesc1, z0, z1, threshold=filter_threshold, kpts0=kpts0, kpts1=kpts1, width=width)

    def get_matchability(self, desc: Tensor) -> Tensor:
        return torch.sigmoid(self.matchability(desc)).squeeze(-1)
