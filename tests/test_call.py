"""pf3plat_amd._call: what the operators' ctypes wrappers share around a library call.  No GPU and no library needed."""
import contextlib

import pytest
import torch

from pf3plat_amd import _call, _lib


def test_f32_converts_only_what_needs_converting():
    """A contiguous float32 tensor comes back as itself - `detach()` makes a new Python object over the same storage, nothing is
    copied -; anything else as a detached contiguous float32 copy."""
    same = torch.arange(12.0).reshape(3, 4).requires_grad_(True)
    out = _call.f32(same)
    assert out.data_ptr() == same.data_ptr() and out.shape == same.shape and out.stride() == same.stride() and not out.requires_grad
    assert out.untyped_storage().data_ptr() == same.untyped_storage().data_ptr()
    for other in (same.double(), same.t(), same.double().t()):
        out = _call.f32(other)
        assert out.dtype == torch.float32 and out.is_contiguous() and not out.requires_grad
        assert out.untyped_storage().data_ptr() != other.untyped_storage().data_ptr()
        assert torch.equal(out, other.detach().to(torch.float32))


def test_ptr_passes_none_through():
    t = torch.zeros(3)
    assert _call.ptr(None) is None and _call.ptr(t) == t.data_ptr()


def test_require_device_refuses_cpu_tensors_with_the_wrappers_messages():
    a, b = torch.zeros(2), torch.zeros(2)
    with pytest.raises(RuntimeError) as e:
        _call.require_device("lift", "lift_depth", (a, b))
    assert str(e.value) == "pf3plat_amd lift: tensors must be on a ROCm device (there is no CPU fallback path)"

    class Placed:  # what the second check reads of a tensor
        is_cuda = True

        def __init__(self, device):
            self.device = device

    with pytest.raises(RuntimeError) as e:
        _call.require_device("lift", "lift_depth", (Placed(torch.device("cuda", 0)), Placed(torch.device("cuda", 1))))
    assert str(e.value) == "lift_depth: every tensor must be on the same device"
    _call.require_device("lift", "lift_depth", [Placed(torch.device("cuda", 1)), Placed(torch.device("cuda", 1))])


def test_scratch_is_never_empty():
    assert _call.scratch(0, torch.float32, "cpu").shape == (1,)
    s = _call.scratch(72, torch.float64, "cpu")
    assert s.shape == (9,) and s.dtype == torch.float64
    assert _call.scratch(7, torch.int64, "cpu").shape == (1,)


def test_launch_loads_at_call_time_appends_the_stream_and_raises_on_a_code(monkeypatch):
    calls = []

    class Lib:
        @staticmethod
        def gsr_fine(*args):
            calls.append(args)
            return 0

        @staticmethod
        def gsr_broken(*args):
            return -1

    monkeypatch.setattr(_lib, "load", lambda: Lib)
    monkeypatch.setattr(_call, "_on_device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(_call, "_stream_ptr", lambda dev: 77)
    assert _call.launch("gsr_fine", "cpu", 1, None, 2.5) is None and calls == [(1, None, 2.5, 77)]
    assert _call.call("gsr_fine", 5, 1) is None and calls[1:] == [(1, 5)]  # the same without the device context: the caller's stream
    with pytest.raises(RuntimeError, match="^gsr_broken failed with code -1$"):
        _call.call("gsr_broken", 5)
    with pytest.raises(RuntimeError) as e:
        _call.launch("gsr_broken", "cpu", 1)
    assert str(e.value) == "gsr_broken failed with code -1"
