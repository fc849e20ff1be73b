"""LightGlue's transformer on the device (reference src/model/LightGlue/lightglue/lightglue.py:133-256, 315-398, 532-538, as
src/model/encoder/encoder_costvolume.py:79 builds it: depth_confidence = width_confidence = -1, no early stop and no pruning): the link
between keypoint extraction (`keypoints.SuperPoint`) and match assignment (`matching.match_assignment`).  Every (pair, scene) list of a
batch lives in ONE packed (T, d) token buffer, T = sum m_l + sum n_l: each projection and FFN runs once over the buffer - the
reference applies the same modules to both images -, and a layer's attention is two `attention.ragged_attention` launches: the
self-attention of both images of every list, q, k and v read out of the interleaved Wqkv output where they lie and rotated by the
positional encoding as they are loaded, and both directions of the cross-attention.  Forward only, as the reference runs the matcher
under no_grad.  The projections, the LayerNorm and the GELU stay torch.
Departures from the reference, all stated in DESIGN.md: float32 where the reference's flash path goes through half precision; `size`
is required (the reference's per-list min/max of `size is None` is left out); no pruning, no early stop, no `add_scale_ori`."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from .attention import MAX_RAGGED_HEAD_DIM, LearnableFourierPositionalEncoding, _ffn, ragged_attention
from .keypoints import PackedKeypoints
from .matching import MatchAssignment, Matches, _offsets, match_assignment


class _SelfParams(nn.Module):
    """The parameters of the reference's SelfBlock under its names: Wqkv, out_proj, ffn.0/1/3."""

    def __init__(self, embed_dim: int) -> None:
        super().__init__()
        self.Wqkv = nn.Linear(embed_dim, 3 * embed_dim, bias=True)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.ffn = _ffn(embed_dim)


class _CrossParams(nn.Module):
    """The parameters of the reference's CrossBlock under its names: to_qk, to_v, to_out, ffn.0/1/3."""

    def __init__(self, embed_dim: int) -> None:
        super().__init__()
        self.to_qk = nn.Linear(embed_dim, embed_dim, bias=True)
        self.to_v = nn.Linear(embed_dim, embed_dim, bias=True)
        self.to_out = nn.Linear(embed_dim, embed_dim, bias=True)
        self.ffn = _ffn(embed_dim)


class ListLayout(NamedTuple):
    """Where the lists lie in the packed buffer: first image's rows of every list, then the second image's."""
    offsets0: tuple   # L + 1 Python ints
    offsets1: tuple
    self_ranges: tuple   # 2 L (begin, count): image 0 of every list, then image 1
    cross_q: tuple       # 2 L: list l's image 0, then its image 1
    cross_k: tuple       # ... and their partners


def list_layout(lengths0: Sequence[int], lengths1: Sequence[int]) -> ListLayout:
    off0, off1 = _offsets(lengths0, "lengths0"), _offsets(lengths1, "lengths1")
    if len(off0) != len(off1) or len(off0) < 2:
        raise ValueError(f"LightGlue: needs as many lengths0 as lengths1 and at least one list, got {len(off0) - 1} and {len(off1) - 1}")
    L, M0 = len(off0) - 1, off0[-1]
    a = tuple((off0[l], off0[l + 1] - off0[l]) for l in range(L))
    b = tuple((M0 + off1[l], off1[l + 1] - off1[l]) for l in range(L))
    cross_q = tuple(r for l in range(L) for r in (a[l], b[l]))
    cross_k = tuple(r for l in range(L) for r in (b[l], a[l]))
    return ListLayout(off0, off1, a + b, cross_q, cross_k)


class TransformerLayer(nn.Module):
    """LightGlue's TransformerLayer (lightglue.py:227-247, the unmasked branch) on the packed buffer: `self_attn` and `cross_attn`
    carry the reference's parameter names, so its state dict loads with strict=True.  forward(x (T, embed_dim), rot (2, T, head_dim),
    layout) -> (T, embed_dim): every linear and FFN once over the buffer, two `ragged_attention` launches."""

    def __init__(self, embed_dim: int, num_heads: int, flash: bool = False) -> None:
        super().__init__()
        if num_heads < 1 or embed_dim % num_heads != 0:
            raise ValueError(f"TransformerLayer: embed_dim {embed_dim} is not a multiple of num_heads {num_heads}")
        if embed_dim // num_heads > MAX_RAGGED_HEAD_DIM:
            raise ValueError(f"TransformerLayer: {embed_dim // num_heads} channels per head; the ragged attention supports at most {MAX_RAGGED_HEAD_DIM}")
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.self_attn = _SelfParams(embed_dim)
        self.cross_attn = _CrossParams(embed_dim)

    @torch.no_grad()
    def forward(self, x: Tensor, rot: Optional[Tensor], layout: ListLayout) -> Tensor:
        if x.dim() != 2 or x.shape[1] != self.embed_dim:
            raise ValueError(f"TransformerLayer: expected the packed buffer (T, {self.embed_dim}), got {tuple(x.shape)}")
        T, H, D = x.shape[0], self.num_heads, self.head_dim
        s, c = self.self_attn, self.cross_attn
        qkv = s.Wqkv(x).view(T, H, D, 3)  # (the reference's unflatten(-1, (H, -1, 3)): q, k, v interleaved along the last axis)
        context = ragged_attention(qkv[..., 0], qkv[..., 1], qkv[..., 2], layout.self_ranges, layout.self_ranges, rot=rot)
        x = x + s.ffn(torch.cat([x, s.out_proj(context.view(T, H * D))], -1))
        qk, v = c.to_qk(x).view(T, H, D), c.to_v(x).view(T, H, D)
        message = ragged_attention(qk, qk, v, layout.cross_q, layout.cross_k, scale=D ** -0.5)
        return x + c.ffn(torch.cat([x, c.to_out(message.view(T, H * D))], -1))


class _TokenConfidence(nn.Module):
    """lightglue.py:77-87, plain torch; never called here (no early stop): it is there so that the reference's state dict loads."""

    def __init__(self, dim: int) -> None:
        super().__init__()
        self.token = nn.Sequential(nn.Linear(dim, 1), nn.Sigmoid())

    def forward(self, desc0: Tensor, desc1: Tensor):
        return self.token(desc0.detach()).squeeze(-1), self.token(desc1.detach()).squeeze(-1)


def normalize_keypoints(kpts: Tensor, size) -> Tensor:
    """lightglue.py:25-36 with a given size (W, H): (kpts - size / 2) / (max(size) / 2)."""
    size = torch.as_tensor(size, device=kpts.device, dtype=kpts.dtype)
    return (kpts - (size / 2)[..., None, :]) / (size.max(-1).values / 2)[..., None, None]


class LightGlue(nn.Module):
    """The reference's LightGlue (lightglue.py:315-398) as the encoder configures it; its state dict loads with strict=True.
    forward(desc0, desc1, kpts0, kpts1, lengths0, lengths1, size, width=None) -> matching.Matches."""

    def __init__(self, input_dim: int = 256, descriptor_dim: int = 256, n_layers: int = 9, num_heads: int = 4, filter_threshold: float = 0.1,
                 depth_confidence: float = -1, width_confidence: float = -1, add_scale_ori: bool = False) -> None:
        super().__init__()
        if depth_confidence != -1 or width_confidence != -1:
            raise ValueError("LightGlue: early stop and point pruning are not supported on the device: depth_confidence and "
                             f"width_confidence must be -1, got {depth_confidence} and {width_confidence}")
        if add_scale_ori:
            raise ValueError("LightGlue: add_scale_ori is not supported on the device")
        if n_layers < 1:
            raise ValueError(f"LightGlue: needs at least one layer, got {n_layers}")
        self.input_dim, self.descriptor_dim, self.n_layers, self.num_heads = input_dim, descriptor_dim, n_layers, num_heads
        self.filter_threshold = filter_threshold
        self.input_proj = nn.Linear(input_dim, descriptor_dim, bias=True) if input_dim != descriptor_dim else nn.Identity()
        head_dim = descriptor_dim // num_heads
        self.posenc = LearnableFourierPositionalEncoding(2, head_dim, head_dim)
        self.transformers = nn.ModuleList([TransformerLayer(descriptor_dim, num_heads) for _ in range(n_layers)])
        self.log_assignment = nn.ModuleList([MatchAssignment(descriptor_dim) for _ in range(n_layers)])
        self.token_confidence = nn.ModuleList([_TokenConfidence(descriptor_dim) for _ in range(n_layers - 1)])
        thresholds = [min(max(0.8 + 0.1 * math.exp(-4.0 * i / n_layers), 0.0), 1.0) for i in range(n_layers)]
        self.register_buffer("confidence_thresholds", torch.tensor(thresholds, dtype=torch.float32))

    def _lists(self, desc0, desc1, kpts0, kpts1, lengths0, lengths1):
        """The packed ragged form of the inputs and, for the equal-length form, (B, m, n)."""
        if (lengths0 is None) != (lengths1 is None):
            raise ValueError("LightGlue: lengths0 and lengths1 go together")
        batch = None
        if lengths0 is None:
            if desc0.dim() != 3 or desc1.dim() != 3 or desc0.shape[0] != desc1.shape[0] or desc0.shape[0] < 1:
                raise ValueError(f"LightGlue: expected desc0 (B, m, d) and desc1 (B, n, d), got {tuple(desc0.shape)}, {tuple(desc1.shape)}")
            batch = (desc0.shape[0], desc0.shape[1], desc1.shape[1])
            lengths0, lengths1 = (batch[1],) * batch[0], (batch[2],) * batch[0]
            desc0, desc1, kpts0, kpts1 = desc0.flatten(0, 1), desc1.flatten(0, 1), kpts0.flatten(0, 1), kpts1.flatten(0, 1)
        layout = list_layout(lengths0, lengths1)
        for name, t, total, width in (("desc0", desc0, layout.offsets0[-1], self.input_dim), ("desc1", desc1, layout.offsets1[-1], self.input_dim),
                                      ("kpts0", kpts0, layout.offsets0[-1], 2), ("kpts1", kpts1, layout.offsets1[-1], 2)):
            if tuple(t.shape) != (total, width):
                raise ValueError(f"LightGlue: expected {name} ({total}, {width}), got {tuple(t.shape)}")
        if layout.offsets0[-1] + layout.offsets1[-1] < 1:
            raise ValueError("LightGlue: no keypoints at all")
        return desc0, desc1, kpts0, kpts1, layout, batch

    @torch.no_grad()
    def encode(self, desc0: Tensor, desc1: Tensor, kpts0: Tensor, kpts1: Tensor, lengths0, lengths1, size) -> Tuple[Tensor, ListLayout]:
        """The descriptors after the last layer, the packed (sum m_l + sum n_l, descriptor_dim) buffer - first images' rows, then the
        second images' -, and its layout."""
        if size is None:
            raise ValueError("LightGlue: size = (W, H) is required (the reference's per-list extent of `size is None` is not supported)")
        desc0, desc1, kpts0, kpts1, layout, _ = self._lists(desc0, desc1, kpts0, kpts1, lengths0, lengths1)
        kpts = normalize_keypoints(torch.cat([kpts0, kpts1]).to(torch.float32), size)
        rot = self.posenc(kpts)[:, 0].contiguous()  # (2, T, head_dim): cosines, sines, each repeated twice
        x = self.input_proj(torch.cat([desc0, desc1]).detach().to(torch.float32))
        for layer in self.transformers:
            x = layer(x, rot, layout)
        return x, layout

    @torch.no_grad()
    def forward(self, desc0: Tensor, desc1: Tensor, kpts0: Tensor, kpts1: Tensor, lengths0: Optional[Sequence[int]] = None,
                lengths1: Optional[Sequence[int]] = None, size=None, width: Optional[int] = None) -> Matches:
        """desc0 (sum m_l, input_dim), desc1 (sum n_l, input_dim), kpts0 (sum m_l, 2), kpts1 (sum n_l, 2) (x, y) in pixels with the
        lists' lengths - or the equal-length (B, m, .) / (B, n, .) form without lengths -, size = (W, H) -> Matches of the lists.  With
        `width` the matches carry pixel ids and points, so that `matching.pack_matched` takes them.  A list with an empty side has no
        matches (its other side still passes through the self-attention; nothing reads the result)."""
        x, layout = self.encode(desc0, desc1, kpts0, kpts1, lengths0, lengths1, size)
        _, _, k0, k1, _, batch = self._lists(desc0, desc1, kpts0, kpts1, lengths0, lengths1)
        M0 = layout.offsets0[-1]
        head = self.log_assignment[-1]
        mdesc, z = head.final_proj(x), head.matchability(x)
        lens = lambda off: tuple(off[l + 1] - off[l] for l in range(len(off) - 1))
        with_kpts = width is not None
        m = match_assignment(mdesc[:M0], mdesc[M0:], z[:M0], z[M0:], lens(layout.offsets0), lens(layout.offsets1), threshold=self.filter_threshold,
                             kpts0=k0 if with_kpts else None, kpts1=k1 if with_kpts else None, width=width)
        if batch is not None:
            B, mm, nn_ = batch
            m = m._replace(matches0=m.matches0.reshape(B, mm), matches1=m.matches1.reshape(B, nn_),
                           matching_scores0=m.matching_scores0.reshape(B, mm), matching_scores1=m.matching_scores1.reshape(B, nn_))
        return m


class PairLists(NamedTuple):
    desc0: Tensor      # (sum m_l, C)
    desc1: Tensor      # (sum n_l, C)
    kpts0: Tensor      # (sum m_l, 2)
    kpts1: Tensor
    lengths0: tuple    # m_l
    lengths1: tuple


def pair_lists(packed: PackedKeypoints, num_scenes: int, num_views: int) -> PairLists:
    """The two sides of every (pair, scene) list out of the packed keypoints of num_scenes x num_views images in (b v) order, in the
    order `matching.pack_matched` expects: list l = pair x num_scenes + scene, pairs (a, b), a < b, in the encoder's order
    (encoder_costvolume.py:323).  Two gathers per array; the row indices come from the lengths: no host read."""
    b, v = int(num_scenes), int(num_views)
    if b < 1 or v < 2 or len(packed.lengths) != b * v:
        raise ValueError(f"pair_lists: {len(packed.lengths)} images are not {num_scenes} scenes x {num_views} >= 2 views")
    if packed.descriptors is None:
        raise ValueError("pair_lists: the keypoints carry no descriptors")
    starts = [0]
    for n in packed.lengths:
        starts.append(starts[-1] + int(n))
    dev = packed.keypoints.device
    rows0, rows1, len0, len1 = [], [], [], []
    for i, j in [(i, j) for i in range(v) for j in range(i + 1, v)]:
        for s in range(b):
            for rows, lens, img in ((rows0, len0, s * v + i), (rows1, len1, s * v + j)):
                rows.append(torch.arange(starts[img], starts[img + 1], device=dev))
                lens.append(starts[img + 1] - starts[img])
    i0, i1 = torch.cat(rows0), torch.cat(rows1)
    return PairLists(packed.descriptors[i0], packed.descriptors[i1], packed.keypoints[i0], packed.keypoints[i1], tuple(len0), tuple(len1))
