"""What every ctypes wrapper of an operator (cost_volume, lift, mono_attention, attention, matching, pose, losses) does around its own checks and
allocations: the float32 view of an input, the device check, a scratch array from a byte count, and the library call on the tensors'
device and torch's current stream.  The rasterizer's path has its own (rasterizer.HipBackend)."""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib
from .rasterizer import _on_device, _ptr as ptr, _stream_ptr  # noqa: F401  (ptr: None stays None, a tensor gives its data_ptr())


def f32(t: Tensor) -> Tensor:
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


def require_device(module: str, function: str, tensors) -> None:
    """The device check of a wrapper, after its shape checks and before the library is loaded."""
    for t in tensors:  # (plain loops: a generator costs more than the checks, and the rays and the refined poses are 10 - 20 us calls)
        if not t.is_cuda:
            raise RuntimeError(f"pf3plat_amd {module}: tensors must be on a ROCm device (there is no CPU fallback path)")
    dev = tensors[0].device
    for t in tensors:
        if t.device != dev:
            raise RuntimeError(f"{function}: every tensor must be on the same device")


def scratch(nbytes: int, dtype, dev) -> Tensor:
    """An uninitialised array of at least `nbytes` (what a gsr_*_scratch_bytes answers), never empty: its data_ptr() is passed on."""
    return torch.empty(max(int(nbytes) // dtype.itemsize, 1), dtype=dtype, device=dev)


def call(name: str, stream: int, *args) -> None:
    """lib.<name>(*args, stream), the library loaded at call time; RuntimeError on a non-zero code.  By itself only where several
    launches share one `with _on_device(dev)` and one stream handle (the image loss and metrics: a launch and its finish)."""
    rc = getattr(_lib.load(), name)(*args, stream)
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}")


def launch(name: str, dev, *args) -> None:
    """`call` with `dev` the current device, on torch's current stream of `dev`."""
    with _on_device(dev):
        call(name, _stream_ptr(dev), *args)
