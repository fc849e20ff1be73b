"""Multi-head attention on the device, and LightGlue's SelfBlock / CrossBlock on top of it: the blocks of the encoder's pose transformer
(reference src/model/LightGlue/lightglue/lightglue.py:133-224 as src/model/encoder/encoder_costvolume.py:401-441 builds and calls them;
the definition of the attention is stated in include/gsr.h).  `multi_head_attention` is one launch forward (gsr_attention) and three
small-state launches backward (gsr_attention_backward): the key axis is streamed with the online softmax, nothing of N x M elements is
formed or saved, operands are read through their strides where they lie and results are token-major.  There is no CPU fallback.  The
projections, the LayerNorm, the GELU and the rotary embedding stay torch."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from ._call import f32, launch, ptr, require_device, scratch

MAX_HEAD_DIM = 32


def _operand(t: Tensor) -> Tensor:
    """The array handed to the library for a (B, H, tokens, D) operand: a float32 tensor of ANY strides is read where it lies (the
    library takes the four element strides), so the reference's interleaved `qkv[..., i]` views and its `.transpose(1, 2)` views are
    not copied; only another dtype is converted."""
    t = t.detach()
    return t if t.dtype == torch.float32 else t.to(torch.float32)


def _strides(t: Tensor):
    return (ctypes.c_int64 * 4)(*t.stride())


def _attention_args(q, k, v, scale):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if q.dim() != 4:
        raise ValueError(f"multi_head_attention: expected q (B, H, N, D), got {tuple(q.shape)}")
    B, H, N, D = q.shape
    if k.dim() != 4 or k.shape[0] != B or k.shape[1] != H or k.shape[3] != D:
        raise ValueError(f"multi_head_attention: expected k (B, H, M, D) = ({B}, {H}, M, {D}), got {tuple(k.shape)}")
    M = k.shape[2]
    if tuple(v.shape) != (B, H, M, D):
        raise ValueError(f"multi_head_attention: expected v (B, H, M, D) = ({B}, {H}, {M}, {D}), got {tuple(v.shape)}")
    if B < 1 or H < 1 or N < 1 or M < 1:
        raise ValueError(f"multi_head_attention: needs B, H, N, M >= 1, got B={B}, H={H}, N={N}, M={M}")
    if not 1 <= D <= MAX_HEAD_DIM:
        raise ValueError(f"multi_head_attention: supports 1 <= D <= {MAX_HEAD_DIM} channels per head, got {D}")
    if B * H * max(N, M) * D > 0x7fffffff:
        raise ValueError("multi_head_attention: more than 2^31 - 1 elements in an array")
    scale = D ** -0.5 if scale is None else float(scale)
    if scale != scale or scale in (float("inf"), float("-inf")):
        raise ValueError(f"multi_head_attention: scale must be finite, got {scale}")
    require_device("attention", "multi_head_attention", (q, k, v))
    return B, H, N, M, D, scale


class _MultiHeadAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        B, H, N, M, D, scale = _attention_args(q, k, v, scale)
        dev, f32 = q.device, torch.float32
        qa, ka, va = _operand(q), _operand(k), _operand(v)
        out = torch.empty((B, N, H, D), dtype=f32, device=dev)  # token-major (both fully written by the call)
        lse = torch.empty((B, H, N), dtype=f32, device=dev)
        launch("gsr_attention", dev, B, H, N, M, D, scale, qa.data_ptr(), _strides(qa), ka.data_ptr(), _strides(ka), va.data_ptr(), _strides(va),
               out.data_ptr(), lse.data_ptr())
        ctx.save_for_backward(q, k, v, out, lse)  # O(B H (N + M) D); nothing of N x M
        ctx.sizes = (B, H, N, M, D, scale)
        return out.permute(0, 2, 1, 3).to(v.dtype)

    @staticmethod
    def backward(ctx, g_out):
        q, k, v, out, lse = ctx.saved_tensors
        B, H, N, M, D, scale = ctx.sizes
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return None, None, None, None
        dev, f32 = q.device, torch.float32
        qa, ka, va = _operand(q), _operand(k), _operand(v)
        g = g_out.detach().permute(0, 2, 1, 3)  # (B, N, H, D): contiguous already when the cotangent came through the transposed view
        if g.dtype != f32 or not g.is_contiguous():
            g = g.to(f32).contiguous()
        d_q = torch.empty((B, N, H, D), dtype=f32, device=dev) if need_q else None  # (fully written by the call)
        d_k = torch.empty((B, M, H, D), dtype=f32, device=dev) if need_k else None
        d_v = torch.empty((B, M, H, D), dtype=f32, device=dev) if need_v else None
        work = scratch(_lib.load().gsr_attention_scratch_bytes(B, H, N, M, D), f32, dev)
        launch("gsr_attention_backward", dev, B, H, N, M, D, scale, qa.data_ptr(), _strides(qa), ka.data_ptr(), _strides(ka), va.data_ptr(),
               _strides(va), out.data_ptr(), lse.data_ptr(), g.data_ptr(), ptr(d_q), ptr(d_k), ptr(d_v), work.data_ptr())
        view = lambda d, like: d.permute(0, 2, 1, 3).to(like.dtype)
        return view(d_q, q) if need_q else None, view(d_k, k) if need_k else None, view(d_v, v) if need_v else None, None


def multi_head_attention(q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None) -> Tensor:
    """q (B, H, N, D), k and v (B, H, M, D), of any strides -> (B, H, N, D): F.scaled_dot_product_attention(q, k, v) without mask or
    dropout, as include/gsr.h defines it; `scale` defaults to D ** -0.5 and multiplies the scores.  1 <= D <= 32.  The result is the
    transposed view of a contiguous (B, N, H, D) buffer, so `.transpose(1, 2).flatten(-2)` costs nothing; the gradients are such views
    as well.  The key axis is streamed with the online softmax: no (N, M) array exists, and the function saves its inputs, the output and
    one log-sum-exp per query.  Differentiable in q, k and v; forward and every gradient are bit-reproducible (no atomics).  One launch
    forward, three backward, no host synchronisation.  float32 operands are read where they lie whatever their strides; other dtypes are
    converted, and the result and the gradients come back in the inputs' dtypes."""
    return _MultiHeadAttention.apply(q, k, v, scale)


def bidirectional_cross_attention(qk0: Tensor, qk1: Tensor, v0: Tensor, v1: Tensor, scale: Optional[float] = None,
                                  need_m1: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """LightGlue's two softmaxes over the one similarity qk0 qk1^T (lightglue.py:210-217), neither the similarity nor an attention
    matrix formed: m0 = multi_head_attention(qk0, qk1, v1), m1 = multi_head_attention(qk1, qk0, v0).  qk0, v0 (B, H, N, D); qk1, v1
    (B, H, M, D).  With need_m1 = False m1 is None and nothing is launched for it."""
    m0 = multi_head_attention(qk0, qk1, v1, scale)
    m1 = multi_head_attention(qk1, qk0, v0, scale) if need_m1 else None
    return m0, m1


MAX_RAGGED_HEAD_DIM = 64


def _ranges(ranges, name: str, T: int):
    begins, counts = [], []
    for r in ranges:
        if len(r) != 2 or int(r[0]) != r[0] or int(r[1]) != r[1]:
            raise ValueError(f"ragged_attention: {name} holds (begin, count) pairs of Python ints, got {r!r}")
        b, c = int(r[0]), int(r[1])
        if b < 0 or c < 0 or b + c > T:
            raise ValueError(f"ragged_attention: {name} range ({b}, {c}) does not lie inside the {T} rows")
        begins.append(b)
        counts.append(c)
    return begins, counts


def _ragged_args(q, k, v, q_ranges, k_ranges, scale, rot):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if q.dim() != 3:
        raise ValueError(f"ragged_attention: expected q (T, H, D), got {tuple(q.shape)}")
    T, H, D = q.shape
    for name, t in (("k", k), ("v", v)):
        if tuple(t.shape) != (T, H, D):
            raise ValueError(f"ragged_attention: expected {name} (T, H, D) = ({T}, {H}, {D}), got {tuple(t.shape)}")
    if T < 1 or H < 1:
        raise ValueError(f"ragged_attention: needs T, H >= 1, got T={T}, H={H}")
    if not 1 <= D <= MAX_RAGGED_HEAD_DIM:
        raise ValueError(f"ragged_attention: supports 1 <= D <= {MAX_RAGGED_HEAD_DIM} channels per head, got {D}")
    if T * H * D > 0x7fffffff:
        raise ValueError("ragged_attention: more than 2^31 - 1 elements in an array")
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != torch.float32:
            raise ValueError(f"ragged_attention: {name} must be float32 (it is read where it lies), got {t.dtype}")
    qb, qc = _ranges(q_ranges, "q_ranges", T)
    kb, kc = _ranges(k_ranges, "k_ranges", T)
    if len(qb) != len(kb) or len(qb) < 1:
        raise ValueError(f"ragged_attention: needs as many q_ranges as k_ranges and at least one unit, got {len(qb)} and {len(kb)}")
    if rot is not None:
        if tuple(rot.shape) != (2, T, D):
            raise ValueError(f"ragged_attention: expected rot (2, T, D) = (2, {T}, {D}), cosines then sines, got {tuple(rot.shape)}")
        if D % 2:
            raise ValueError(f"ragged_attention: a rotary encoding needs an even D, got {D}")
    scale = D ** -0.5 if scale is None else float(scale)
    if scale != scale or scale in (float("inf"), float("-inf")):
        raise ValueError(f"ragged_attention: scale must be finite, got {scale}")
    require_device("attention", "ragged_attention", [q, k, v] + ([rot] if rot is not None else []))
    return T, H, D, scale, (qb, qc, kb, kc)


@torch.no_grad()
def ragged_attention(q: Tensor, k: Tensor, v: Tensor, q_ranges: Sequence[Tuple[int, int]], k_ranges: Sequence[Tuple[int, int]],
                     scale: Optional[float] = None, rot: Optional[Tensor] = None, out: Optional[Tensor] = None, return_lse: bool = False):
    """Softmax attention of U units over ONE packed row space, as include/gsr.h defines it (gsr_ragged_attention): q, k, v (T, H, D)
    float32 of any strides, read where they lie; unit u attends its query rows q_ranges[u] = (begin, count) to its key rows
    k_ranges[u]; 1 <= D <= 64; `scale` defaults to D ** -0.5.  `rot` (2, T, D), cosines then sines, rotates q and k (not v) while they
    are loaded, as `apply_cached_rotary_emb`.  Returns contiguous (T, H, D): rows of a unit without keys are zero, rows no unit owns
    keep what `out` held (zeros when `out` is not given); with return_lse also the (H, T) log-sum-exp of the scores, -inf for a unit
    without keys, unwritten for rows no unit owns.  Forward only, as the reference runs the matcher under no_grad.  One launch
    for all units and heads, nothing of n x m elements, no host synchronisation, the same bits on every call.  There is no CPU fallback."""
    T, H, D, scale, arrays = _ragged_args(q, k, v, q_ranges, k_ranges, scale, rot)
    dev, U = q.device, len(arrays[0])
    qa, ka, va = q.detach(), k.detach(), v.detach()
    ra = f32(rot) if rot is not None else None
    if out is None:
        out = torch.zeros((T, H, D), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (T, H, D) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"ragged_attention: out must be a contiguous float32 ({T}, {H}, {D}) on the operands' device")
    lse = torch.empty((H, T), dtype=torch.float32, device=dev)
    host = [(ctypes.c_int32 * U)(*a) for a in arrays]
    both = torch.tensor(arrays, dtype=torch.int32)
    both = both.pin_memory().to(dev, non_blocking=True)  # (from Python ints: goes up without waiting)
    work = scratch(_lib.load().gsr_ragged_attention_scratch_bytes(U, T, H, D, *host), torch.float32, dev)
    s3 = lambda t: (ctypes.c_int64 * 3)(*t.stride())
    launch("gsr_ragged_attention", dev, U, T, H, D, scale, host[0], both[0].data_ptr(), host[1], both[1].data_ptr(), host[2],
           both[2].data_ptr(), host[3], both[3].data_ptr(), qa.data_ptr(), s3(qa), ka.data_ptr(), s3(ka), va.data_ptr(), s3(va), ptr(ra),
           out.data_ptr(), lse.data_ptr(), work.data_ptr())
    return (out, lse) if return_lse else out


def rotate_half(x: Tensor) -> Tensor:
    x = x.unflatten(-1, (-1, 2))
    x1, x2 = x.unbind(dim=-1)
    return torch.stack((-x2, x1), dim=-1).flatten(start_dim=-2)


def apply_cached_rotary_emb(freqs: Tensor, t: Tensor) -> Tensor:
    """The reference's rotation of channel pairs by the cached (cos, sin) of an encoding (lightglue.py:57-58); plain torch."""
    return (t * freqs[0]) + (rotate_half(t) * freqs[1])


class LearnableFourierPositionalEncoding(nn.Module):
    """lightglue.py:61-74, plain torch: positions (..., M) -> the (2, ..., 1, N, F_dim) stack of cosines and sines, each repeated twice."""

    def __init__(self, M: int, dim: int, F_dim: Optional[int] = None, gamma: float = 1.0) -> None:
        super().__init__()
        F_dim = F_dim if F_dim is not None else dim
        self.gamma = gamma
        self.Wr = nn.Linear(M, F_dim // 2, bias=False)
        nn.init.normal_(self.Wr.weight.data, mean=0, std=self.gamma ** -2)

    def forward(self, x: Tensor) -> Tensor:
        projected = self.Wr(x)
        emb = torch.stack([torch.cos(projected), torch.sin(projected)], 0).unsqueeze(-3)
        return emb.repeat_interleave(2, dim=-1)


def _ffn(embed_dim: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(2 * embed_dim, 2 * embed_dim), nn.LayerNorm(2 * embed_dim, elementwise_affine=True), nn.GELU(),
                         nn.Linear(2 * embed_dim, embed_dim))


def _head_dim(name: str, embed_dim: int, num_heads: int) -> int:
    if num_heads < 1 or embed_dim % num_heads != 0:
        raise ValueError(f"{name}: embed_dim {embed_dim} is not a multiple of num_heads {num_heads}")
    if embed_dim // num_heads > MAX_HEAD_DIM:
        raise ValueError(f"{name}: {embed_dim // num_heads} channels per head; the device attention supports at most {MAX_HEAD_DIM}")
    return embed_dim // num_heads


class SelfBlock(nn.Module):
    """LightGlue's SelfBlock (lightglue.py:133-166) with the reference's parameter names (Wqkv, out_proj, ffn.0/1/3: its state dict
    loads with strict=True) and its forward signature; the attention is `multi_head_attention`, which reads q, k and v out of the
    interleaved Wqkv output where they lie (a rotary encoding makes q and k arrays of their own, as in the reference).  `flash` is
    accepted and runs the same float32 path: the reference would go through half precision there.  Masks are not supported."""

    def __init__(self, embed_dim: int, num_heads: int, flash: bool = False, bias: bool = True) -> None:
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.head_dim = _head_dim("SelfBlock", embed_dim, num_heads)
        self.Wqkv = nn.Linear(embed_dim, 3 * embed_dim, bias=bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.ffn = _ffn(embed_dim)

    def forward(self, x: Tensor, encoding: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> Tensor:
        if mask is not None:
            raise NotImplementedError("SelfBlock: attention masks are not supported on the device")
        qkv = self.Wqkv(x).unflatten(-1, (self.num_heads, -1, 3)).transpose(1, 2)
        q, k, v = qkv[..., 0], qkv[..., 1], qkv[..., 2]
        if encoding is not None:
            q = apply_cached_rotary_emb(encoding, q)
            k = apply_cached_rotary_emb(encoding, k)
        context = multi_head_attention(q, k, v)
        message = self.out_proj(context.transpose(1, 2).flatten(start_dim=-2))
        return x + self.ffn(torch.cat([x, message], -1))


class CrossBlock(nn.Module):
    """LightGlue's CrossBlock (lightglue.py:169-224) with the reference's parameter names (to_qk, to_v, to_out, ffn.0/1/3: its state
    dict loads with strict=True); the two attentions over the shared similarity are `bidirectional_cross_attention`.  `need_x1=False`
    returns (x0', None) and skips the second attention, the second to_out and the second ffn - the encoder's `feat_others, _ = ...`
    (encoder_costvolume.py:437), with identical values and gradients for what is kept.  `flash` is accepted and runs the same float32
    path: the reference would go through half precision there.  Masks are not supported."""

    def __init__(self, embed_dim: int, num_heads: int, flash: bool = False, bias: bool = True) -> None:
        super().__init__()
        self.heads = num_heads
        dim_head = _head_dim("CrossBlock", embed_dim, num_heads)
        self.scale = dim_head ** -0.5
        inner_dim = dim_head * num_heads
        self.to_qk = nn.Linear(embed_dim, inner_dim, bias=bias)
        self.to_v = nn.Linear(embed_dim, inner_dim, bias=bias)
        self.to_out = nn.Linear(inner_dim, embed_dim, bias=bias)
        self.ffn = _ffn(embed_dim)

    def forward(self, x0: Tensor, x1: Tensor, mask: Optional[Tensor] = None, need_x1: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
        if mask is not None:
            raise NotImplementedError("CrossBlock: attention masks are not supported on the device")
        heads = lambda t: t.unflatten(-1, (self.heads, -1)).transpose(1, 2)
        qk0, qk1 = heads(self.to_qk(x0)), heads(self.to_qk(x1))
        v0, v1 = (heads(self.to_v(x0)) if need_x1 else None), heads(self.to_v(x1))
        if need_x1:
            m0, m1 = bidirectional_cross_attention(qk0, qk1, v0, v1, self.scale)
        else:
            m0, m1 = multi_head_attention(qk0, qk1, v1, self.scale), None
        m0 = self.to_out(m0.transpose(1, 2).flatten(start_dim=-2))
        x0 = x0 + self.ffn(torch.cat([x0, m0], -1))
        if m1 is None:
            return x0, None
        m1 = self.to_out(m1.transpose(1, 2).flatten(start_dim=-2))
        return x0, x1 + self.ffn(torch.cat([x1, m1], -1))
