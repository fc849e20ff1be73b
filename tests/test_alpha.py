"""Accumulated alpha (A = 1 - T_final) without a GPU: the two new entry points of the C ABI (gsr_forward_alpha /
gsr_backward_alpha) are declared, exported and bound with the argument lists of the _ex calls plus one pointer each; ABI number, the
pinned structs, the flag mask and every workspace size are what they were; the Python surface has the switch, off by default."""
import ctypes
import inspect
import os
import re

import torch

from pf3plat_amd import _lib, decoder, rasterizer, splatting
from pf3plat_amd.types import DecoderOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(name):
    """Parameter names of function `name` as include/gsr.h declares it."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    body = re.search(r"\bint %s\s*\((.*?)\);" % name, hdr, re.S).group(1)
    return [re.search(r"(\w+)\s*$", a.strip()).group(1) for a in body.split(",")]


def test_alpha_entry_points_are_the_ex_calls_plus_one_pointer():
    lib = _lib.load()
    fwd, bwd = _params("gsr_forward_ex"), _params("gsr_backward_ex")
    assert _params("gsr_forward_alpha") == fwd[:fwd.index("out_extra") + 1] + ["out_alpha"] + fwd[fwd.index("out_extra") + 1:]
    assert _params("gsr_backward_alpha") == bwd[:bwd.index("dL_dextra_img") + 1] + ["dL_dalpha_img"] + bwd[bwd.index("dL_dextra_img") + 1:]
    for name, ex in (("gsr_forward_alpha", lib.gsr_forward_ex), ("gsr_backward_alpha", lib.gsr_backward_ex)):
        fn = getattr(lib, name)  # exported by the built library
        assert name in _lib.EXPORTED_SYMBOLS and fn.restype is ctypes.c_int
        assert len(fn.argtypes) == len(_params(name)) == len(ex.argtypes) + 1
        assert fn.argtypes[0] is ex.argtypes[0] and fn.argtypes[-2:] == ex.argtypes[-2:]  # dims first; options, stream last
        assert all(t is ctypes.c_void_p for t in fn.argtypes[1:-2])


def test_alpha_entry_points_validate_like_the_ex_calls():
    """Host-only answers (nothing is launched): bad dims are refused, an empty call is fine."""
    lib = _lib.load()
    be = rasterizer.HipBackend()
    cfg = rasterizer.RasterConfig(1, 1, 1, 16, 8, 8, 0, 0)
    null = [None] * 13
    for flags in (0x100000, 1 << 30, 0x100):  # no new flag bit came with the feature: the mask is what it was
        dims = be._dims(rasterizer.RasterConfig(1, 1, 1, 16, 8, 8, 0, 0, 4, False, flags), 1024)
        assert lib.gsr_forward_alpha(ctypes.byref(dims), *null, None, None) == -1
        assert lib.gsr_backward_alpha(ctypes.byref(dims), *null, *[None] * 6, None, None) == -1
        assert lib.gsr_workspace_sizes(ctypes.byref(dims), None, None, None) == -1
    empty = be._dims(rasterizer.RasterConfig(0, 0, 1, 16, 8, 8, 0, 0), 1024)
    assert lib.gsr_forward_alpha(ctypes.byref(empty), *null, None, None) == 0
    assert lib.gsr_backward_alpha(ctypes.byref(empty), *null, *[None] * 6, None, None) == 0
    dims = be._dims(cfg, 1024)
    assert lib.gsr_forward_alpha(ctypes.byref(dims), *null, None, None) == -1  # (views, image and workspaces are required)


def test_abi_number_structs_and_sizes_are_unchanged():
    lib = _lib.load()
    assert lib.gsr_abi_version() == _lib.GSR_ABI_VERSION == 4
    assert ctypes.sizeof(_lib.GsrDims) == 56 and ctypes.sizeof(_lib.GsrForwardOptions) == 24 and ctypes.sizeof(_lib.GsrBackwardOptions) == 48
    assert [n for n, _ in _lib.GsrForwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "stage_ms"]
    assert [n for n, _ in _lib.GsrBackwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "dL_dviews", "pose_partials", "stage_ms",
                                                                "depth_term_only", "reserved_"]
    # the request sizes nothing: a call shape with and without it has the same dims, hence the same workspaces
    be = rasterizer.HipBackend()
    plain = rasterizer.RasterConfig(3, 1, 3, 1000, 72, 40, 4, 25, 4, True, 1 << 4)
    wanted = rasterizer.RasterConfig(3, 1, 3, 1000, 72, 40, 4, 25, 4, True, 1 << 4, False, True)
    assert wanted.alpha and not plain.alpha
    assert bytes(be._dims(plain, 1 << 16)) == bytes(be._dims(wanted, 1 << 16))
    assert rasterizer._cfg_vec(plain) + [1] == rasterizer._cfg_vec(wanted) and len(rasterizer._cfg_vec(plain)) == 12


def test_python_surface_has_the_switch_off_by_default():
    color, depth = torch.zeros(1, 1, 3, 2, 2), torch.zeros(1, 1, 2, 2)
    assert DecoderOutput(color, depth).alpha is None
    assert DecoderOutput(color, None).alpha is None
    assert DecoderOutput(color, depth, depth).alpha is depth
    assert [f for f in DecoderOutput.__dataclass_fields__] == ["color", "depth", "alpha"]
    assert inspect.signature(rasterizer.rasterize_views).parameters["return_alpha"].default is False
    assert inspect.signature(splatting.render_views).parameters["alpha"].default is False
    assert inspect.signature(decoder.DecoderSplattingCUDA.forward).parameters["alpha"].default is False
    assert "alpha" not in inspect.signature(splatting.render_cuda).parameters  # (the reference-shaped wrappers keep their shapes)
