"""The depth predictor's "multi guided by mono" attention on the device (reference
src/model/encoder/costvolume/depth_predictor_multiview.py:360-366; the definition is stated in include/gsr.h):
`mono_guided_attention` replaces softmax(mono_q mono_k) applied to multi_v - two batched products around an (n, L, L) softmax, 512 MiB
per copy at PF3plat's size - by one launch forward (gsr_mono_attention) and three small-state launches backward
(gsr_mono_attention_backward).  Nothing of L x L elements is formed or saved.  There is no CPU fallback."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib
from ._call import f32, launch, ptr, require_device, scratch


def _channel_major_q(mono_q: Tensor) -> Tensor:
    """(n, L, E) -> the (n, E, L) contiguous array of the same values: the permuted view of the reference's line 360 (strides
    (E L, 1, L)) is read where it lies; any other layout is copied once."""
    qt = mono_q.detach().permute(0, 2, 1)
    return qt if qt.dtype == torch.float32 and qt.is_contiguous() else qt.to(torch.float32).contiguous()


def _attention_args(mono_q, mono_k, multi_v):
    """The shape checks (before the device is looked at and before the library is loaded), then the device check."""
    if mono_q.dim() != 3:
        raise ValueError(f"mono_guided_attention: expected mono_q (n, L, E), got {tuple(mono_q.shape)}")
    n, L, E = mono_q.shape
    if tuple(mono_k.shape) != (n, E, L):
        raise ValueError(f"mono_guided_attention: expected mono_k (n, E, L) = ({n}, {E}, {L}), got {tuple(mono_k.shape)}")
    if multi_v.dim() != 3 or multi_v.shape[0] != n or multi_v.shape[2] != L:
        raise ValueError(f"mono_guided_attention: expected multi_v (n, C, L) = ({n}, C, {L}), got {tuple(multi_v.shape)}")
    C = multi_v.shape[1]
    if n < 1 or L < 1:
        raise ValueError(f"mono_guided_attention: needs n >= 1 and L >= 1, got n={n}, L={L}")
    if not 1 <= E <= 32:
        raise ValueError(f"mono_guided_attention: supports 1 <= E <= 32 score channels, got {E}")
    if not 1 <= C <= 256:
        raise ValueError(f"mono_guided_attention: supports 1 <= C <= 256 value channels, got {C}")
    if n * max(E, C) * L > 0x7fffffff:
        raise ValueError("mono_guided_attention: more than 2^31 - 1 elements in an array")
    require_device("mono_attention", "mono_guided_attention", (mono_q, mono_k, multi_v))
    return n, E, L, C


class _MonoGuidedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mono_q, mono_k, multi_v):
        n, E, L, C = _attention_args(mono_q, mono_k, multi_v)
        dev = mono_q.device
        q, k, v = _channel_major_q(mono_q), f32(mono_k), f32(multi_v)
        out = torch.empty((n, C, L), dtype=torch.float32, device=dev)  # (both fully written by the call)
        lse = torch.empty((n, L), dtype=torch.float32, device=dev)
        launch("gsr_mono_attention", dev, n, E, L, C, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr())
        ctx.save_for_backward(mono_q, mono_k, multi_v, out, lse)  # O(n L (E + C)); nothing of L x L
        ctx.sizes = (n, E, L, C)
        return out.to(multi_v.dtype)

    @staticmethod
    def backward(ctx, g_out):
        mono_q, mono_k, multi_v, out, lse = ctx.saved_tensors
        n, E, L, C = ctx.sizes
        need_q, need_k, need_v = ctx.needs_input_grad
        if not (need_q or need_k or need_v):
            return None, None, None
        dev = mono_q.device
        q, k, v, g = _channel_major_q(mono_q), f32(mono_k), f32(multi_v), f32(g_out)
        d_q = torch.empty((n, E, L), dtype=torch.float32, device=dev) if need_q else None  # (fully written by the call)
        d_k = torch.empty((n, E, L), dtype=torch.float32, device=dev) if need_k else None
        d_v = torch.empty((n, C, L), dtype=torch.float32, device=dev) if need_v else None
        work = scratch(_lib.load().gsr_mono_attention_scratch_bytes(n, E, L, C), torch.float32, dev)
        launch("gsr_mono_attention_backward", dev, n, E, L, C, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
               g.data_ptr(), ptr(d_q), ptr(d_k), ptr(d_v), work.data_ptr())
        return (d_q.permute(0, 2, 1).to(mono_q.dtype) if need_q else None, d_k.to(mono_k.dtype) if need_k else None,
                d_v.to(multi_v.dtype) if need_v else None)


def mono_guided_attention(mono_q: Tensor, mono_k: Tensor, multi_v: Tensor) -> Tensor:
    """mono_q (n, L, E), mono_k (n, E, L), multi_v (n, C, L) -> (n, C, L): torch.bmm(multi_v, softmax(torch.bmm(mono_q, mono_k),
    dim=-1).permute(0, 2, 1)) as include/gsr.h defines it - the reference's tensors as they stand, no 1 / sqrt(E) factor.  mono_q with
    strides (E L, 1, L), the permuted view of the reference's line 360, is read where it lies; any other layout is copied to
    channel-major once.  1 <= E <= 32, 1 <= C <= 256.  The key axis is streamed with the online softmax: no (L, L) array exists, and
    the function saves its inputs, the output and one log-sum-exp per query.  Differentiable in all three inputs; the forward and
    every gradient are bit-reproducible (no atomics).  One launch forward, three backward, no host synchronisation.  Inputs that are
    not float32 or not contiguous are converted; the result and the gradients come back in the inputs' dtypes."""
    return _MonoGuidedAttention.apply(mono_q, mono_k, multi_v)
