"""Accumulated alpha (A = 1 - T_final) without a GPU: the image and its cotangent are the last fields of the launch options structs
(GsrForwardOptions.out_alpha / GsrBackwardOptions.dL_dalpha_img) and no entry point takes either as a parameter; the _ex calls
validate as before when the options carry the pointer; the flag mask and every workspace size are what they were; the Python surface
has the switch, off by default."""
import ctypes
import dataclasses
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


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)


def _struct_fields(name):
    """Field names of struct `name` as include/gsr.h declares it, in order."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), re.S).group(1)
    return [re.search(r"(\w+)\s*(\[\w+\])?\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]


def test_alpha_pointers_are_the_last_option_fields_and_no_parameter():
    lib = _lib.load()
    assert _struct_fields("GsrForwardOptions")[-1] == "out_alpha" == _lib.GsrForwardOptions._fields_[-1][0]
    assert _struct_fields("GsrBackwardOptions")[-1] == "dL_dalpha_img" == _lib.GsrBackwardOptions._fields_[-1][0]
    functions = re.findall(r"\b(gsr_\w+)\s*\(([^;{}]*?)\)\s*;", _header(), re.S)
    assert {"gsr_forward", "gsr_backward", "gsr_forward_ex", "gsr_backward_ex"} <= {n for n, _ in functions}
    for name, params in functions:
        assert not re.search(r"\b(out_alpha|dL_dalpha_img)\b", params), name
    for name in ("gsr_forward_ex", "gsr_backward_ex"):  # the one entry point each way that carries the options
        fn = getattr(lib, name)  # exported by the built library
        assert name in _lib.EXPORTED_SYMBOLS and fn.restype is ctypes.c_int and len(fn.argtypes) == len(_params(name))
        assert _params(name)[-2:] == ["opt", "stream"] and all(t is ctypes.c_void_p for t in fn.argtypes[1:-2])
    assert lib.gsr_forward_ex.argtypes[-2]._type_ is _lib.GsrForwardOptions and lib.gsr_backward_ex.argtypes[-2]._type_ is _lib.GsrBackwardOptions


def test_ex_calls_validate_with_an_alpha_pointer_in_their_options():
    """Host-only answers (nothing is launched, no pointer is followed): bad dims are refused, an empty call is fine."""
    lib = _lib.load()
    be = rasterizer.HipBackend()
    cfg = rasterizer.RasterConfig(1, 1, 1, 16, 8, 8, 0, 0)
    image = (ctypes.c_float * 64)()  # (a non-null address for the alpha fields)
    fopt = _lib.GsrForwardOptions(None, 0, 0, None, ctypes.addressof(image))
    bopt = _lib.GsrBackwardOptions(None, 0, 0, None, None, None, 0, 0, ctypes.addressof(image))
    assert fopt.out_alpha and bopt.dL_dalpha_img
    fnull, bnull = [None] * 12, [None] * 18
    for flags in (0x100000, 1 << 30, 0x100):  # no new flag bit came with the feature: the mask is what it was
        dims = be._dims(rasterizer.RasterConfig(1, 1, 1, 16, 8, 8, 0, 0, 4, False, flags), 1024)
        assert lib.gsr_forward_ex(ctypes.byref(dims), *fnull, ctypes.byref(fopt), None) == -1
        assert lib.gsr_backward_ex(ctypes.byref(dims), *bnull, ctypes.byref(bopt), None) == -1
        assert lib.gsr_workspace_sizes(ctypes.byref(dims), None, None, None) == -1
    empty = be._dims(rasterizer.RasterConfig(0, 0, 1, 16, 8, 8, 0, 0), 1024)
    assert lib.gsr_forward_ex(ctypes.byref(empty), *fnull, ctypes.byref(fopt), None) == 0
    assert lib.gsr_backward_ex(ctypes.byref(empty), *bnull, ctypes.byref(bopt), None) == 0
    dims = be._dims(cfg, 1024)
    assert lib.gsr_forward_ex(ctypes.byref(dims), *fnull, ctypes.byref(fopt), None) == -1  # (views, image and workspaces are required)
    assert lib.gsr_backward_ex(ctypes.byref(dims), *bnull, ctypes.byref(bopt), None) == -1


def test_the_request_sizes_nothing_and_is_the_last_entry_of_the_call_shape():
    lib = _lib.load()
    assert lib.gsr_abi_version() == _lib.GSR_ABI_VERSION == 5
    assert ctypes.sizeof(_lib.GsrDims) == 56 and ctypes.sizeof(_lib.GsrForwardOptions) == 32 and ctypes.sizeof(_lib.GsrBackwardOptions) == 56
    assert [n for n, _ in _lib.GsrForwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "stage_ms", "out_alpha"]
    assert [n for n, _ in _lib.GsrBackwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "dL_dviews", "pose_partials", "stage_ms",
                                                                "depth_term_only", "reserved_", "dL_dalpha_img"]
    # the request sizes nothing: a call shape with and without it has the same dims, hence the same workspaces
    be = rasterizer.HipBackend()
    plain = rasterizer.RasterConfig(3, 1, 3, 1000, 72, 40, 4, 25, 4, True, 1 << 4)
    wanted = rasterizer.RasterConfig(3, 1, 3, 1000, 72, 40, 4, 25, 4, True, 1 << 4, False, True)
    assert wanted.alpha and not plain.alpha
    assert bytes(be._dims(plain, 1 << 16)) == bytes(be._dims(wanted, 1 << 16))
    ext = _lib.load_torch_ext()
    assert dataclasses.fields(rasterizer.RasterConfig)[-1].name == ext.CFG_FIELDS[-1] == "alpha"
    assert plain != wanted and dataclasses.replace(plain, alpha=True) == wanted  # they differ in that field alone
    assert bytes(ext.launch_dims(plain, 1 << 16)) == bytes(ext.launch_dims(wanted, 1 << 16))


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
