"""GSR_FLAG_FOV_GRADIENT and gsr_setup_views_backward_ex, as far as the built library answers without a GPU: the flag's value and
what it sizes, the new symbol and its argument checks - and the guard of the camera-rig case the GPU module
(tests/test_gpu_fov_gradient.py) measures the tan-fov gradient on, checked against the oracles alone."""
import ctypes
import inspect
import re

import numpy as np

from pf3plat_amd import _lib
from tests import camera_rig, fov_rig

BASE = dict(num_views=2, num_sets=1, views_per_set=2, num_gaussians=100, height=64, width=80, sh_degree=4, sh_coeffs=25, max_sh_eval=4,
            has_extra=1, flags=0, pair_capacity=1 << 16)


def _dims(**kw):
    f = dict(BASE, **kw)
    return _lib.GsrDims(_lib.GSR_ABI_VERSION, *(f[k] for k in list(BASE)))


def _sizes(lib, d):
    g, b, i = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.gsr_workspace_sizes(ctypes.byref(d), ctypes.byref(g), ctypes.byref(b), ctypes.byref(i))
    return rc, (g.value, b.value, i.value)


def test_flag_value_and_what_it_sizes():
    with open(_lib.HEADER) as f:
        header = f.read()
    assert re.search(r"#define\s+GSR_FLAG_FOV_GRADIENT\s+0x200000\b", header)
    assert _lib.FLAG_FOV_GRADIENT == 0x200000
    lib = _lib.load()
    fov = _lib.FLAG_FOV_GRADIENT
    for flags in (0, _lib.FLAG_BACKWARD_FOLLOWS, _lib.FLAG_DETERMINISTIC, _lib.FLAG_BACKWARD_FOLLOWS | _lib.FLAG_DETERMINISTIC):
        rc0, s0 = _sizes(lib, _dims(flags=flags))
        rc1, s1 = _sizes(lib, _dims(flags=flags | fov))
        assert rc0 == 0 and rc1 == 0 and s0 == s1 and all(s0)
        d0, d1 = _dims(flags=flags), _dims(flags=flags | fov)
        assert lib.gsr_backward_scratch_bytes(ctypes.byref(d0)) == lib.gsr_backward_scratch_bytes(ctypes.byref(d1)) > 0
    for n in (100, 64, 65):
        d0, d1 = _dims(num_gaussians=n), _dims(num_gaussians=n, flags=fov)
        rows = 2 * (-(-n // 64) * 4 + 256)
        assert lib.gsr_pose_partials_bytes(ctypes.byref(d0)) == rows * 35 * 4
        assert lib.gsr_pose_partials_bytes(ctypes.byref(d1)) == rows * 37 * 4


def test_abi_and_options_structs_are_what_they_were():
    assert _lib.load().gsr_abi_version() == 5 == _lib.GSR_ABI_VERSION
    assert ctypes.sizeof(_lib.GsrForwardOptions) == 32 and ctypes.sizeof(_lib.GsrBackwardOptions) == 56
    assert [n for n, _ in _lib.GsrForwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "stage_ms", "out_alpha"]
    assert [n for n, _ in _lib.GsrBackwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "dL_dviews", "pose_partials", "stage_ms",
                                                                "depth_term_only", "reserved_", "dL_dalpha_img"]


def test_setup_views_backward_ex_is_exported_and_checks_its_arguments():
    assert "gsr_setup_views_backward_ex" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    fn = lib.gsr_setup_views_backward_ex
    buf = (ctypes.c_float * 64)()  # (never read: every call below returns before a launch)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert fn(-1, p, p, p, p, p, None) == -1
    assert fn(1, None, p, p, p, p, None) == -1
    assert fn(1, p, None, p, p, p, None) == -1 and fn(1, p, p, None, p, p, None) == -1
    assert fn(0, None, None, None, None, None, None) == 0


def test_the_request_is_a_keyword_that_defaults_to_off():
    from pf3plat_amd import decoder, rasterizer, splatting

    for fn in (rasterizer.views_from_cameras, rasterizer.rasterize_views, splatting.render_cuda, splatting.render_views,
               decoder.DecoderSplattingCUDA.forward):
        assert inspect.signature(fn).parameters["intrinsics_gradients"].default is False, fn
    assert list(inspect.signature(rasterizer.views_from_cameras).parameters)[-2:] == ["pose_gradients", "intrinsics_gradients"]


def test_the_gpu_tests_case_meets_its_guard():
    """The condition tests/test_gpu_fov_gradient.py rests on: the seed guard of the rig; a live clamp term in every view; central
    differences of the fp64 forward over tanfovx, tanfovy that agree between two steps to the bar tests/test_oracle_pose_grad.py holds the
    oracle's analytic camera gradient to; and a gradient large enough to measure against."""
    c = fov_rig.guarded_case()
    assert c.cfg.num_gaussians <= 3000 and c.cfg.num_views == 3 and (c.cfg.height, c.cfg.width) == (64, 80) and c.want_views is True
    ref = camera_rig.rig_case(**fov_rig.CASE)
    assert np.array_equal(c.gc.numpy(), ref.gc.numpy()) and np.array_equal(c.ge.numpy(), ref.ge.numpy())  # the case's own cotangents
    o32, o64 = camera_rig.oracle_pair(c)
    camera_rig.seed_guard(c, o32, o64)
    pop = camera_rig.population(c, o32["radii"])
    assert all(row["clamped"] > 0 for row in pop), pop
    fd_a, fd_b = fov_rig.reference()
    assert fov_rig.STEPS == (1e-6, 5e-7) and fd_a.shape == (3, 2)
    big = np.maximum(np.abs(fd_a), np.abs(fd_b)).max(axis=1, keepdims=True)  # per view: the scale the GPU test's error is taken at
    print("fd(1e-6)", fd_a.tolist(), "fd(5e-7)", fd_b.tolist(), "clamped", [row["clamped"] for row in pop])
    assert (np.abs(fd_a - fd_b) <= 2e-6 * big).all(), (fd_a, fd_b)
    assert (np.abs(fd_a).max(axis=1) > 1e-3).all(), fd_a
    # the torch surface's reference: differences over fx, fy, cx, cy through the float64 set-up, held to the same agreement
    ia, ib = fov_rig.intrinsics_reference()
    big = np.maximum(np.abs(ia), np.abs(ib)).max(axis=1, keepdims=True)
    assert ia.shape == (3, 4) and (np.abs(ia - ib) <= 2e-6 * big).all(), (ia, ib)
    assert (np.abs(ia).max(axis=1) > 1e-3).all(), ia
