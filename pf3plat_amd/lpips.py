"""The perceptual distance of PF3plat's training loss and evaluation (reference src/loss/loss_lpips.py and `compute_lpips`,
src/evaluation/metrics.py:27-33, which call `lpips.LPIPS(net="vgg")`): the VGG16 convolutions stay in torch (MIOpen), everything
after them - the channel normalisation of five feature pyramids, the weighted squared difference, the spatial mean - is ONE
operator of the raster library (`gsr_lpips_head`, `gsr_lpips_head_finish`, `gsr_lpips_head_backward`; definition in include/gsr.h):
two launches forward and one backward for all layers, where the eager lines make about ten passes over the largest tensors of
the training step.  One departure from the package, stated in include/gsr.h: the gradient of a feature vector that is entirely
zero is 0, where autograd returns NaN.  No CPU fallback: tensors must be on a ROCm device.
"""
from __future__ import annotations

import ctypes
from typing import Mapping, Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from ._call import call, f32, require_device
from .rasterizer import _on_device, _stream_ptr

MAX_LAYERS = _lib.LPIPS_MAX_LAYERS
MAX_CHANNELS = 1024
VGG_CHANNELS = (64, 128, 256, 512, 512)
# torchvision's vgg16().features: the convolutions' indices, per slice; a 2 x 2 max-pool opens slices 2 to 5
VGG_SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
_VGG_WIDTHS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
               (512, 512), (512, 512), (512, 512))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def _table(fa: Sequence[Tensor], fb: Sequence[Tensor], ws: Sequence[Tensor]) -> "_lib.GsrLpipsLayers":
    t = _lib.GsrLpipsLayers()
    t.num_layers = len(fa)
    for l, (a, b, w) in enumerate(zip(fa, fb, ws)):
        row = t.layer[l]
        row.a, row.b, row.weight = a.data_ptr(), b.data_ptr(), w.data_ptr()
        row.channels, row.height, row.width = a.shape[1], a.shape[2], a.shape[3]
    return t


def _check(features_a, features_b, weights) -> int:
    """The shape checks (before the device is looked at and before the library is loaded), then the device check -> N."""
    L = len(features_a)
    if not (1 <= L <= MAX_LAYERS) or len(features_b) != L or len(weights) != L:
        raise ValueError(f"lpips_distance: expected 1 to {MAX_LAYERS} layers and as many on either side and of weights, got "
                         f"{len(features_a)}, {len(features_b)}, {len(weights)}")
    n = features_a[0].shape[0] if features_a[0].dim() == 4 else -1
    for l, (a, b, w) in enumerate(zip(features_a, features_b, weights)):
        if a.dim() != 4 or a.shape != b.shape or a.shape[0] != n:
            raise ValueError(f"lpips_distance: layer {l}: expected two equal (n, c, h, w) feature maps of the same n, got {tuple(a.shape)} and {tuple(b.shape)}")
        c = a.shape[1]
        if not (1 <= c <= MAX_CHANNELS) or a.shape[2] < 1 or a.shape[3] < 1 or a.shape[2] * a.shape[3] > 0x7fffffff:
            raise ValueError(f"lpips_distance: layer {l}: 1 to {MAX_CHANNELS} channels on at least one pixel, got {tuple(a.shape)}")
        if w.numel() != c:
            raise ValueError(f"lpips_distance: layer {l}: {c} channels but {w.numel()} weights")
    require_device("lpips", "lpips_distance", (*features_a, *features_b, *weights))
    return n


class _LpipsHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, num_layers, *tensors):
        L = num_layers
        fa, fb, ws = tensors[:L], tensors[L:2 * L], tensors[2 * L:]
        n = _check(fa, fb, ws)
        lib = _lib.load()
        dev = fa[0].device
        values = torch.empty(n, dtype=torch.float32, device=dev)  # (the finish writes every element of both)
        per_layer = torch.empty((n, MAX_LAYERS), dtype=torch.float32, device=dev)
        ctx.num_layers, ctx.empty = L, n == 0
        ctx.mark_non_differentiable(per_layer)
        if n == 0:
            return values, per_layer
        a32, b32, w32 = [f32(t) for t in fa], [f32(t) for t in fb], [f32(t).reshape(-1) for t in ws]
        table = _table(a32, b32, w32)
        slots = int(lib.gsr_lpips_head_partials(n, table))
        if slots == 0:
            raise RuntimeError("gsr_lpips_head refuses these sizes (more than 16 777 215 units of work)")
        partials = torch.empty(slots, dtype=torch.float32, device=dev)
        stream = _stream_ptr(dev)
        with _on_device(dev):
            call("gsr_lpips_head", stream, n, table, partials.data_ptr())
            call("gsr_lpips_head_finish", stream, n, table, partials.data_ptr(), values.data_ptr(), per_layer.data_ptr())
        ctx.save_for_backward(*fa, *fb, *ws)
        return values, per_layer

    @staticmethod
    def backward(ctx, g_values, _g_per_layer):
        L = ctx.num_layers
        need = ctx.needs_input_grad[1:]
        if ctx.empty:
            return (None,) * (1 + 3 * L)
        saved = ctx.saved_tensors
        fa, fb, ws = saved[:L], saved[L:2 * L], saved[2 * L:]
        a32, b32, w32 = [f32(t) for t in fa], [f32(t) for t in fb], [f32(t).reshape(-1) for t in ws]
        dev = a32[0].device
        n = a32[0].shape[0]
        da = [torch.empty_like(a32[l]) if need[l] else None for l in range(L)]
        db = [torch.empty_like(b32[l]) if need[L + l] else None for l in range(L)]
        if any(t is not None for t in (*da, *db)):
            pa = (ctypes.c_void_p * MAX_LAYERS)(*[None if t is None else t.data_ptr() for t in da])
            pb = (ctypes.c_void_p * MAX_LAYERS)(*[None if t is None else t.data_ptr() for t in db])
            g = f32(g_values)
            with _on_device(dev):
                call("gsr_lpips_head_backward", _stream_ptr(dev), n, _table(a32, b32, w32), g.data_ptr(), pa, pb)
        return (None, *[None if t is None else t.to(fa[l].dtype) for l, t in enumerate(da)],
                *[None if t is None else t.to(fb[l].dtype) for l, t in enumerate(db)], *([None] * L))


def lpips_distance(features_a: Sequence[Tensor], features_b: Sequence[Tensor], weights: Sequence[Tensor]):
    """One to five layers of feature maps (n, c_l, h_l, w_l) on either side and c_l non-negative weights per layer ->
    (values (n,), per_layer (n, 5)): per image the sum over the layers of the spatial mean of sum_c w_c (a^_c - b^_c)^2, a^ = a /
    (|a| + 1e-10) along the channels, and the layers' terms (zeros in the columns past the last layer; no gradient).
    Differentiable in the features of whichever side requires it (the weights receive none); two launches forward, one backward,
    no host synchronisation.  The gradient of an all-zero feature vector is 0 (autograd of the eager lines: NaN).  Inputs that are
    not float32 or not contiguous are converted."""
    features_a, features_b, weights = list(features_a), list(features_b), list(weights)
    return _LpipsHead.apply(len(features_a), *features_a, *features_b, *weights)


# ------------------------------------------------------------------------------------------------------------------------
# The module: scaling layer, VGG16 features, five `lin` weight vectors
# ------------------------------------------------------------------------------------------------------------------------
def _conv_name(index: int) -> str:
    return f"conv{index}"


class LPIPS(torch.nn.Module):
    """`lpips.LPIPS(net="vgg")`, version 0.1, eval mode: `forward(in0, in1, normalize=False)` -> (n, 1, 1, 1).  The scaling layer
    and the 13 VGG16 convolutions (plain nn.functional conv2d / relu / max_pool2d: torchvision is not needed) run in torch; the
    distance head is `lpips_distance`.  The module is always in eval mode and every tensor of it is a NON-PERSISTENT buffer (the
    reference's `convert_to_buffer(..., persistent=False)`): nothing of it trains, gradients flow to the images, and its `state_dict()`
    is empty, so a training wrapper's checkpoints neither carry the 58 MB of VGG weights nor expect them.

    NO PRETRAINED WEIGHTS SHIP WITH THE PROJECT AND NONE ARE FETCHED.  Without a state dict the module holds SEEDED RANDOM weights
    (Kaiming-normal convolutions, zero biases, uniform [0, 1) `lin` weights; `seed`): its values are then self-consistent but are
    not the published metric's.  For those, pass the package's state dict (`state_dict=` or `load_lpips_state_dict`)."""

    def __init__(self, state_dict: Optional[Mapping[str, Tensor]] = None, seed: int = 0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.register_buffer("shift", torch.tensor(SHIFT).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("scale", torch.tensor(SCALE).view(1, 3, 1, 1), persistent=False)
        indices = [i for s in VGG_SLICES for i in s]
        for i, (cin, cout) in zip(indices, _VGG_WIDTHS):
            w = torch.randn((cout, cin, 3, 3), generator=gen) * (2.0 / (cin * 9)) ** 0.5
            self.register_buffer(_conv_name(i) + "_weight", w, persistent=False)
            self.register_buffer(_conv_name(i) + "_bias", torch.zeros(cout), persistent=False)
        for k, c in enumerate(VGG_CHANNELS):
            self.register_buffer(f"lin{k}", torch.rand(c, generator=gen), persistent=False)
        super().train(False)
        if state_dict is not None:
            self.load_lpips_state_dict(state_dict)

    def train(self, mode: bool = True):
        return super().train(False)  # always in eval mode

    def load_lpips_state_dict(self, state: Mapping[str, Tensor]) -> "LPIPS":
        """The package's key names: scaling_layer.{shift,scale}; net.slice{1..5}.{index}.{weight,bias} with torchvision's indices
        (slice1: 0, 2; slice2: 5, 7; slice3: 10, 12, 14; slice4: 17, 19, 21; slice5: 24, 26, 28); lin{0..4}.model.1.weight of shape
        (1, C, 1, 1).  The `lins.{k}.model.1.weight` aliases of the same tensors are ignored; anything else missing or unexpected is
        an error, and so is a wrong shape."""
        expected = {"scaling_layer.shift": self.shift, "scaling_layer.scale": self.scale}
        for k, s in enumerate(VGG_SLICES):
            for i in s:
                expected[f"net.slice{k + 1}.{i}.weight"] = getattr(self, _conv_name(i) + "_weight")
                expected[f"net.slice{k + 1}.{i}.bias"] = getattr(self, _conv_name(i) + "_bias")
        for k in range(len(VGG_CHANNELS)):
            expected[f"lin{k}.model.1.weight"] = getattr(self, f"lin{k}")
        given = {k: v for k, v in state.items() if not k.startswith("lins.")}
        missing, unexpected = sorted(set(expected) - set(given)), sorted(set(given) - set(expected))
        if missing or unexpected:
            raise RuntimeError(f"load_lpips_state_dict: missing keys {missing}, unexpected keys {unexpected}")
        for k, buf in expected.items():
            if given[k].numel() != buf.numel() or (given[k].dim() == buf.dim() and given[k].shape != buf.shape):
                raise RuntimeError(f"load_lpips_state_dict: {k} has shape {tuple(given[k].shape)}, expected {buf.numel()} elements as {tuple(buf.shape)}")
        with torch.no_grad():
            for k, buf in expected.items():
                buf.copy_(given[k].detach().reshape(buf.shape))
        return self

    def features(self, x: Tensor) -> list:
        """(n, 3, h, w), already in [-1, 1] -> the five taps after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3."""
        F = torch.nn.functional
        x = (x - self.shift) / self.scale
        taps = []
        for k, s in enumerate(VGG_SLICES):
            if k > 0:
                x = F.max_pool2d(x, kernel_size=2, stride=2)
            for i in s:
                x = F.relu(F.conv2d(x, getattr(self, _conv_name(i) + "_weight"), getattr(self, _conv_name(i) + "_bias"), padding=1))
            taps.append(x)
        return taps

    def lin_weights(self) -> list:
        return [getattr(self, f"lin{k}") for k in range(len(VGG_CHANNELS))]

    def forward(self, in0: Tensor, in1: Tensor, normalize: bool = False) -> Tensor:
        if in0.shape != in1.shape or in0.dim() != 4 or in0.shape[1] != 3:
            raise ValueError(f"LPIPS: expected two (n, 3, h, w) images, got {tuple(in0.shape)} and {tuple(in1.shape)}")
        if in0.shape[2] < 16 or in0.shape[3] < 16:
            raise ValueError(f"LPIPS: the fifth tap needs h, w >= 16, got {in0.shape[2]} x {in0.shape[3]}")
        require_device("lpips", "LPIPS.forward", (in0, in1, self.shift))
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        values, _ = lpips_distance(self.features(in0), self.features(in1), self.lin_weights())
        return values.reshape(-1, 1, 1, 1)


def load_lpips_state_dict(module: LPIPS, state: Mapping[str, Tensor]) -> LPIPS:
    """`module.load_lpips_state_dict(state)`: the package's key names, strictly (see there)."""
    return module.load_lpips_state_dict(state)
