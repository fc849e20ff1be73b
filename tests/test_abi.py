"""The C-ABI library loads here (no GPU) and exports every symbol include/gsr.h declares; host-only entry points
(version, workspace sizing, argument validation) behave; the product refuses to run without a ROCm device."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

from pf3plat_amd import _lib, rasterizer
from tests.util import install_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "gsr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _declared_functions()
    assert {"gsr_forward", "gsr_backward", "gsr_mark_visible", "gsr_workspace_sizes", "gsr_abi_version"} <= set(names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/gsr.h but not exported by libgsr_hip.so"
    assert set(_lib.EXPORTED_SYMBOLS) <= set(names)
    assert lib.gsr_abi_version() == _lib.GSR_ABI_VERSION == 5
    assert b"gfx950" in lib.gsr_build_info() and b"abi5" in lib.gsr_build_info()
    # ABI 4: one extended launch entry point each way; the per-feature variants of ABI 3 are neither declared nor exported.  ABI 5: nor
    # are the two calls that took the accumulated alpha as a parameter - an optional image or cotangent is a field of the options
    assert {"gsr_forward_ex", "gsr_backward_ex", "gsr_stage_name"} <= set(names) & set(_lib.EXPORTED_SYMBOLS)
    for n in ("gsr_forward_scale_rot", "gsr_backward_scale_rot", "gsr_forward_profile", "gsr_backward_profile",
              "gsr_forward_alpha", "gsr_backward_alpha"):
        assert n not in names and n not in _lib.EXPORTED_SYMBOLS and not hasattr(lib, n), n


def test_stage_names_are_the_librarys():
    """gsr_stage_name is the one statement of the names a failed debug-mode stage is reported with."""
    lib = _lib.load()
    assert [lib.gsr_stage_name(0, i) for i in range(5)] == [b"colour", b"preprocess/binning", b"count + scans", b"emit", b"per-tile sort + blend"]
    assert [lib.gsr_stage_name(1, i) for i in range(2)] == [b"blend_bwd", b"preprocess_bwd"]
    assert lib.gsr_stage_name(0, -1) is None and lib.gsr_stage_name(0, 5) is None
    assert lib.gsr_stage_name(1, -1) is None and lib.gsr_stage_name(1, 2) is None
    assert len(_lib.FWD_STAGES) == 5 and len(_lib.BWD_STAGES) == 2 and not hasattr(_lib, "FWD_DEBUG_STAGES")


def test_source_stamp_covers_every_file_the_library_is_built_from(tmp_path):
    """One byte changed in gsr_hip.hip, in a header next to it or in include/gsr.h changes the stamp build() compares; the torch
    binding, a library of its own, does not.  On a copy of the sources: nothing is written into the tree."""
    import shutil

    shutil.copytree(os.path.dirname(_lib.SRC), tmp_path / "csrc")
    shutil.copy(_lib.HEADER, tmp_path / "gsr.h")

    def stamp():
        return _lib._source_stamp(csrc=str(tmp_path / "csrc"), header=str(tmp_path / "gsr.h"))

    assert stamp() == _lib._source_stamp()  # the copy is the tree
    before = stamp()
    (tmp_path / "csrc" / "gsr_stage.h").write_bytes(b"// a header gsr_hip.hip would include\n")
    assert stamp() != before, "a new file next to gsr_hip.hip does not make the library stale"
    for path in [tmp_path / "csrc" / "gsr_hip.hip", tmp_path / "csrc" / "gsr_stage.h", tmp_path / "gsr.h"]:
        before, data = stamp(), path.read_bytes()
        path.write_bytes(data[:-1] + b" ")
        assert stamp() != before, f"a change to {path.name} does not make the library stale"
        path.write_bytes(data)
        assert stamp() == before
    with open(tmp_path / "csrc" / "gsr_torch.cpp", "ab") as f:
        f.write(b"\n")
    assert stamp() == before
    # (preprocess_bwd.inc: the text of k_preprocess_bwd, which gsr_hip.hip compiles twice)
    assert {os.path.basename(s) for s in _lib.hip_sources()} == {
        "gsr_hip.hip", "gsr_common.h", "gsr_binning.h", "gsr_tiles_fwd.h", "gsr_backward.h", "gsr_cameras.h", "gsr_covariance.h",
        "gsr_image.h", "gsr_adapter.h", "gsr_pose_loss.h", "gsr_cost_volume.h", "gsr_lift.h", "gsr_mono_attention.h", "gsr_attention.h",
        "gsr_pnp_solver.h", "gsr_coarse_pose.h", "gsr_pose_refine.h", "preprocess_bwd.inc", "gsr.h"}
    with open(_lib.SRC) as f:  # every kernel lives in a header
        assert not [line for line in f if "__global__" in line]
    # ... and the stamp's file set IS the include graph of gsr_hip.hip: no file in csrc/ that changes the stamp without being
    # compiled, no include the stamp misses (includes resolve relative to the including file)
    reached, todo = set(), [os.path.realpath(_lib.SRC)]
    while todo:
        path = todo.pop()
        if path not in reached:
            reached.add(path)
            with open(path) as f:
                todo += [os.path.realpath(os.path.join(os.path.dirname(path), inc)) for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M)]
    assert reached == {os.path.realpath(s) for s in _lib.hip_sources()}


def test_oracle_twin_is_rebuilt_by_content_of_its_sources(tmp_path):
    """The CPU twin refuses dims of another GSR_ABI_VERSION than its header's, so a twin left from another header must not survive:
    its staleness stamp hashes include/gsr.h and the oracle's sources (a copied tree does not keep the order of modification times)."""
    import shutil

    from oracle import gsr_oracle

    gsr_oracle.load_oracle()
    here = os.path.join(ROOT, "oracle")
    src = [os.path.join(here, f) for f in ("gsr_oracle.cpp", "gsr_oracle.hpp", "gsr_cpu.h", "Makefile")] + [_lib.HEADER]
    with open(os.path.join(here, "libgsr_oracle.so.stamp")) as f:
        assert f.read().strip() == gsr_oracle._source_stamp(src)  # the loaded twin is the one of these sources
    hdr = tmp_path / "gsr.h"
    shutil.copy(_lib.HEADER, hdr)
    assert gsr_oracle._source_stamp(src[:-1] + [str(hdr)]) == gsr_oracle._source_stamp(src)
    hdr.write_text(hdr.read_text().replace("#define GSR_ABI_VERSION 5", "#define GSR_ABI_VERSION 4"))
    assert gsr_oracle._source_stamp(src[:-1] + [str(hdr)]) != gsr_oracle._source_stamp(src)


def test_struct_layouts_match_header():
    assert ctypes.sizeof(_lib.GsrDims) == 56  # 12 x int32 + int64
    assert rasterizer.VIEW_FLOATS * 4 == 192  # sizeof(GsrView)
    # the options of the _ex calls: the numbers of the static_assert next to forward_impl (csrc/gsr_hip.hip); no implicit padding
    assert ctypes.sizeof(_lib.GsrForwardOptions) == 32 == sum(ctypes.sizeof(t) for _, t in _lib.GsrForwardOptions._fields_)
    assert ctypes.sizeof(_lib.GsrBackwardOptions) == 56 == sum(ctypes.sizeof(t) for _, t in _lib.GsrBackwardOptions._fields_)
    assert [n for n, _ in _lib.GsrForwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "stage_ms", "out_alpha"]
    assert [n for n, _ in _lib.GsrBackwardOptions._fields_] == ["frames", "num_frames", "scale_rot", "dL_dviews", "pose_partials", "stage_ms",
                                                                "depth_term_only", "reserved_", "dL_dalpha_img"]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    for struct in (_lib.GsrForwardOptions, _lib.GsrBackwardOptions):  # field for field, in the header's order
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct.__name__, hdr, re.S).group(1)
        assert re.findall(r"(\w+);", body) == [n for n, _ in struct._fields_]


def test_workspace_sizes_and_validation():
    lib = _lib.load()
    be = rasterizer.HipBackend()
    cfg = rasterizer.RasterConfig(1, 1, 1, 300000, 256, 256, 4, 25, 4, False)
    dims = be._dims(cfg, 2_000_000)
    g, b, i = be.workspace_sizes(dims)
    assert g >= 300000 * (32 + 16) and i >= 2 * 256 * 256 * 4  # 32-byte records + 16-byte colours
    assert b >= 2_000_000 * 12  # 8-byte keys + 4-byte sorted indices per pair
    lay = be.workspace_layout(dims)
    assert lay["status"] == 0 and lay["keys"] % 256 == 0 and lay["point_list"] > lay["keys"]
    # geom: 32-byte records; the footprint words exist only for the windowed binning chain; sub-arrays on 2 MiB boundaries
    gl = be.geom_layout(dims)
    assert gl["record_bytes"] == 32 and gl["aux"] == -1 and gl["rows"] == -1
    assert gl["rgbc"] >= 300000 * 32 and gl["rgbc"] % (2 << 20) == 0
    wdims = be._dims(rasterizer.RasterConfig(1, 1, 1, 300000, 256, 256, 4, 25, 4, False,
                                             _lib.FLAG_WINDOWED_BINNING | _lib.FLAG_BACKWARD_FOLLOWS), 2_000_000)
    wl = be.geom_layout(wdims)
    assert wl["aux"] >= 300000 * 32 and wl["rgbc"] >= wl["aux"] + 300000 * 16 and wl["rows"] >= wl["rgbc"] + 300000 * 16
    assert all(wl[k] % (2 << 20) == 0 for k in ("aux", "rgbc", "rows"))
    assert be.workspace_sizes(wdims)[0] >= wl["rows"] + 300000 * 48
    # bad arguments are rejected with an error code, never a crash
    bad = be._dims(cfg, 10)
    bad.abi_version = 99
    z = ctypes.c_size_t()
    assert lib.gsr_workspace_sizes(ctypes.byref(bad), ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == -1
    bad = be._dims(rasterizer.RasterConfig(3, 2, 2, 10, 8, 8, 0, 0), 10)  # 3 views != 2 sets x 2
    assert lib.gsr_workspace_sizes(ctypes.byref(bad), ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == -1
    assert lib.gsr_forward(ctypes.byref(bad), *([None] * 13)) == -1
    assert lib.gsr_backward(ctypes.byref(bad), *([None] * 19)) == -1
    # ... and by the extended calls with NULL options, as by the plain ones
    assert lib.gsr_forward_ex(ctypes.byref(bad), *([None] * 12), None, None) == -1
    assert lib.gsr_backward_ex(ctypes.byref(bad), *([None] * 18), None, None) == -1
    # dims of an earlier ABI are refused everywhere: by every helper and every launch
    opts = _lib.GsrForwardOptions(None, 0, 1), _lib.GsrBackwardOptions(None, 0, 1)
    for version in (3, 4):
        old = be._dims(cfg, 2_000_000)
        assert lib.gsr_workspace_sizes(ctypes.byref(old), ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == 0
        old.abi_version = version
        ref, offs = ctypes.byref(old), (ctypes.c_int64 * 8)()
        assert lib.gsr_workspace_sizes(ref, ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == -1
        assert lib.gsr_workspace_layout(ref, offs) == -1 and lib.gsr_geom_layout(ref, offs) == -1
        assert lib.gsr_capacity_for(ref, 1000, 10) == -1 and lib.gsr_colour_in_binning(ref) == -1
        assert lib.gsr_backward_scratch_bytes(ref) == 0 and lib.gsr_pose_partials_bytes(ref) == 0
        assert lib.gsr_mark_visible(ref, None, None, None, None) == -1
        assert lib.gsr_forward(ref, *([None] * 13)) == -1 and lib.gsr_backward(ref, *([None] * 19)) == -1
        assert lib.gsr_forward_ex(ref, *([None] * 12), None, None) == -1 and lib.gsr_backward_ex(ref, *([None] * 18), None, None) == -1
        assert lib.gsr_forward_ex(ref, *([None] * 12), ctypes.byref(opts[0]), None) == -1
        assert lib.gsr_backward_ex(ref, *([None] * 18), ctypes.byref(opts[1]), None) == -1


def test_binning_chunk_follows_the_shape_of_the_call():
    """Gaussians per binning workgroup (choose_chunk, csrc/gsr_common.h), read back from the layout: the pair matrix holds views x rows x
    (tiles + 8) entries of 8 bytes between `counts` and `tile_total`.  One round of workgroups on the 256 CUs where it exists (the
    headline: 247 of 1216; configs[3]: 82 x 3 of 1600; one 131 072-Gaussian view: 256 of 512) - and for calls of several rounds (PF3plat's
    training batch: 4 scenes x 3 views) the chunk whose rounds cost least with the fixed part of a round counted: 1600, not 1024."""
    be = rasterizer.HipBackend()

    def rows(views, sets, n):
        dims = be._dims(rasterizer.RasterConfig(views, sets, views // sets, n, 256, 256, 4, 25, 4, False), 8 * views * n)
        lay = be.workspace_layout(dims)
        per_row = (1024 + 8) * 8
        r = (lay["tile_total"] - lay["counts"]) // (views * per_row)
        assert 0 <= (lay["tile_total"] - lay["counts"]) - r * views * per_row < 256  # (the region is padded to 256 bytes)
        return r

    assert rows(1, 1, 300000) == 247       # chunk 1216
    assert rows(3, 1, 131072) == 82        # chunk 1600: 246 workgroups, one round
    assert rows(1, 1, 131072) == 256       # chunk 512: one round of small workgroups
    assert rows(12, 4, 131072) == 82       # four rounds of 1600 (six rounds of 1024 measured slower)
    assert rows(6, 2, 131072) == 82


def test_flag_bits_are_validated_and_ablation_switches_are_not_in_the_product_library():
    """Unknown GsrDims.flags bits are rejected; the measurement-only ablation / phase-stamp switches (0x100 .. 0x2000, only in
    a -DGSR_ABLATE build made by tools/ablate.py) are unknown bits to the shipped library; extra modes above 4 do not exist."""
    lib = _lib.load()
    be = rasterizer.HipBackend()
    z = ctypes.c_size_t()
    sizes = lambda d: lib.gsr_workspace_sizes(ctypes.byref(d), ctypes.byref(z), ctypes.byref(z), ctypes.byref(z))
    ok = (_lib.FLAG_PREFILTERED | _lib.FLAG_DEBUG | _lib.FLAG_SH_PLANAR | _lib.FLAG_COV_3X3 | _lib.FLAG_DETERMINISTIC |
          _lib.FLAG_BACKWARD_FOLLOWS | _lib.FLAG_FULL_LISTS | (4 << 4))
    assert sizes(be._dims(rasterizer.RasterConfig(1, 1, 1, 100, 16, 16, 4, 25, 4, True, ok), 1000)) == 0
    for bad in (0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x8000, 0x40000, 1 << 30, 5 << 4, 7 << 4):
        assert sizes(be._dims(rasterizer.RasterConfig(1, 1, 1, 100, 16, 16, 4, 25, 4, True, bad), 1000)) == -1, hex(bad)
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    product, _, _ = hdr.partition("#ifdef GSR_ABLATE")
    assert "GSR_FLAG_ABLATE" not in product and "GSR_FLAG_DEBUG_TIMING" not in product
    # scratch sizing of the backward: 12 floats per (view, Gaussian); in deterministic mode 12 x 8 bytes and, behind the rows, one
    # 4-byte word per view (the view's largest cotangent, the unit its fixed-point sums are kept in)
    d = be._dims(rasterizer.RasterConfig(2, 1, 2, 100, 16, 16, 4, 25, 4, False), 1000)
    assert lib.gsr_backward_scratch_bytes(ctypes.byref(d)) == 2 * 100 * 12 * 4
    d = be._dims(rasterizer.RasterConfig(2, 1, 2, 100, 16, 16, 4, 25, 4, False, _lib.FLAG_DETERMINISTIC), 1000)
    assert lib.gsr_backward_scratch_bytes(ctypes.byref(d)) == 2 * 100 * 12 * 8 + 2 * 4
    assert lib.gsr_last_failed_stage() == -1
    # a forward that announces its backward keeps the accumulator rows inside geom
    plain, with_rows = ctypes.c_size_t(), ctypes.c_size_t()
    d0 = be._dims(rasterizer.RasterConfig(2, 1, 2, 100, 16, 16, 4, 25, 4, False), 1000)
    d1 = be._dims(rasterizer.RasterConfig(2, 1, 2, 100, 16, 16, 4, 25, 4, False, _lib.FLAG_BACKWARD_FOLLOWS), 1000)
    assert lib.gsr_workspace_sizes(ctypes.byref(d0), ctypes.byref(plain), ctypes.byref(z), ctypes.byref(z)) == 0
    assert lib.gsr_workspace_sizes(ctypes.byref(d1), ctypes.byref(with_rows), ctypes.byref(z), ctypes.byref(z)) == 0
    assert with_rows.value - plain.value >= 2 * 100 * 12 * 4


def test_no_cpu_fallback_path():
    """The product path must fail loudly off-device (there is no CPU fallback and it never reaches for the oracle)."""
    import pf3plat_amd
    from pf3plat_amd import synthetic

    old = install_backend(None)  # make sure the real backend is what gets constructed
    try:
        sc = synthetic.make_scene(1, 32, (16, 16))
        g = sc.gaussians
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pf3plat_amd.render_cuda(sc.extrinsics[0], sc.intrinsics[0], sc.near[0], sc.far[0], (16, 16), sc.background[None],
                                    g.means, g.covariances, g.harmonics, g.opacities)
        assert isinstance(rasterizer.get_backend(), rasterizer.HipBackend)
    finally:
        install_backend(old)
    import sys

    src = "".join(open(os.path.join(ROOT, "pf3plat_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "pf3plat_amd")) if f.endswith(".py"))
    assert "import oracle" not in src and "from oracle" not in src and "from tests" not in src


def test_rasterizer_argument_errors_match_upstream_messages(oracle_backend):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

    eye = torch.eye(4)
    s = GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, eye, eye, 0, torch.zeros(3), False, False)
    r = GaussianRasterizer(s)
    m = torch.zeros(2, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), cov3D_precomp=torch.zeros(2, 6))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.ones(2, 1), colors_precomp=torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):
        r(means3D=torch.zeros(2, 4), means2D=m, opacities=torch.ones(2, 1), colors_precomp=torch.zeros(2, 3), cov3D_precomp=torch.zeros(2, 6))


def test_capacity_for_is_host_arithmetic():
    """gsr_capacity_for: 2 x max(num_pairs, views x tiles x slot), slot = min(max_list, max(2 x mean list, 256)) - half the index
    list is per-(view, tile) slots, half a shared region for the longer lists (include/gsr.h)."""
    lib = _lib.load()
    be = rasterizer.HipBackend()
    cfg = rasterizer.RasterConfig(3, 1, 3, 1000, 256, 256, 4, 25, 4, False)
    dims = be._dims(cfg, 0)
    vt = 3 * 4 * 16 * 16  # views x 8x8 tiles of a 256 x 256 image
    assert lib.gsr_capacity_for(ctypes.byref(dims), 5_000_000, 100) == 2 * 5_000_000
    assert lib.gsr_capacity_for(ctypes.byref(dims), 1000, 2000) == 2 * vt * 256  # sparse scene, one long list: the floor
    assert lib.gsr_capacity_for(ctypes.byref(dims), 1000, 100) == 2 * vt * 100  # every list fits the longest
    mean = -(-3_000_000 // vt)
    assert lib.gsr_capacity_for(ctypes.byref(dims), 3_000_000, 50_000) == 2 * vt * 2 * mean  # skewed: twice the mean, not the outlier
    assert lib.gsr_capacity_for(ctypes.byref(dims), 3_000_000, 50_000) <= 4 * 3_000_000 + 4 * vt
    assert be.capacity_for(cfg, {"num_pairs": 1000, "max_list": 100}, headroom=1.0) == 2 * vt * (100 + 16)
    dims.abi_version = 99
    assert lib.gsr_capacity_for(ctypes.byref(dims), 1, 1) == -1
    # covariance helpers: bad sizes / null pointers are error codes, n == 0 is a no-op
    assert lib.gsr_cov_from_scale_rot(-1, None, None, ctypes.c_float(1.0), None, None) == -1
    assert lib.gsr_cov_from_scale_rot(0, None, None, ctypes.c_float(1.0), None, None) == 0
    assert lib.gsr_cov_from_scale_rot(4, None, None, ctypes.c_float(1.0), None, None) == -1
    assert lib.gsr_cov_from_scale_rot_backward(4, None, None, ctypes.c_float(1.0), None, None, None, None) == -1


def test_geom_sub_arrays_never_overlap_and_fit_the_reported_size():
    """Host-side layout arithmetic over random shapes and flags: records, (windowed) footprint words, colours, (announced
    backward) accumulator rows and saved Jacobians follow each other without overlap inside gsr_workspace_sizes' geom bytes."""
    import numpy as np

    be = rasterizer.HipBackend()
    rng = np.random.default_rng(11)
    for _ in range(200):
        sets = int(rng.integers(1, 4))
        vps = int(rng.integers(1, 5))
        v = sets * vps
        n = int(rng.choice([1, 63, 1000, 131072, 300000, 1_000_000]))
        h, w = int(rng.integers(1, 1200)), int(rng.integers(1, 1200))
        k = int(rng.choice([0, 1, 4, 9, 16, 25]))
        flags = 0
        if rng.random() < 0.3:
            flags |= _lib.FLAG_WINDOWED_BINNING
        if rng.random() < 0.5:
            flags |= _lib.FLAG_BACKWARD_FOLLOWS
        deg = {0: 0, 1: 0, 4: 1, 9: 2, 16: 3, 25: 4}[k]
        cfg = rasterizer.RasterConfig(v, sets, vps, n, h, w, deg, k, 4, False, flags)
        dims = be._dims(cfg, 4 * n + 1024)
        g = be.workspace_sizes(dims)[0]
        gl = be.geom_layout(dims)
        t8 = 4 * ((w + 15) // 16) * ((h + 15) // 16)
        windowed = bool(flags & _lib.FLAG_WINDOWED_BINNING) or t8 > 20480
        assert gl["record_bytes"] == 32
        end = v * n * 32
        if windowed:
            assert gl["aux"] >= end
            end = gl["aux"] + v * n * 16
        else:
            assert gl["aux"] == -1
        assert gl["rgbc"] >= end
        end = gl["rgbc"] + v * n * 16
        if flags & _lib.FLAG_BACKWARD_FOLLOWS:
            assert gl["rows"] >= end
            end = gl["rows"] + v * n * 48 + (v * n * 48 if k > 0 else 0)  # rows, then d rgb / d direction
        else:
            assert gl["rows"] == -1
        assert g >= end, (cfg, g, end, gl)


def test_compiled_torch_binding_loads_and_carries_the_policy_defaults():
    """The torch-facing path is ONE compiled translation unit (pf3plat_amd/csrc/gsr_torch.cpp -> pf3plat_amd/_gsr_torch.so, built by
    __graft_entry__.build()): it loads in-tree, resolves the C ABI out of libgsr_hip.so, exposes the autograd entry points the package
    calls, and a fresh backend object carries the default pair-count policy (host logic only - no compute without a GPU)."""
    import os

    ext = _lib.load_torch_ext()
    assert os.path.dirname(ext.__file__) == os.path.dirname(_lib.LIB_PATH)  # in-tree: it travels with the snapshot
    for name in ("Backend", "rasterize", "rasterize_one_view", "views_from_cameras", "setup_views", "pack_view", "init"):
        assert hasattr(ext, name), name
    be = rasterizer.HipBackend()
    assert (be.sync_policy, be.defer_after, be.on_overflow, be.defer_status) == ("sync", 4, "raise", False)
    assert (be.spin_us, be.headroom_min, be.headroom_max, be.headroom_sigmas) == (300.0, 1.25, 3.0, 4.0)
    assert be.pending == [] and be.seen == {} and be.capacity_hint == {} and be.last_status is None and not be.poisoned
    be.sync_policy, be.defer_after, be.on_overflow = "lazy", 0, "nan"
    assert (be._c.sync_policy, be._c.defer_after, be._c.on_overflow) == ("lazy", 0, "nan")
    with pytest.raises(ValueError):
        be.sync_policy = "sometimes"
    with pytest.raises(ValueError):
        be.on_overflow = "ignore"
    assert (be.sync_policy, be.on_overflow) == ("lazy", "nan")  # (a rejected value leaves the knob as it was)
    # the capacity of a status block with the default 1.25 x head-room is the C ABI's arithmetic on the scaled counts
    cfg = rasterizer.RasterConfig(3, 1, 3, 131072, 256, 256, 4, 25, 4, True, 1 << 4)
    st = {"num_pairs": 1645303, "overflow": 0, "max_list": 766}
    lib = _lib.load()
    dims = be._dims(cfg, 0)
    assert be.capacity_for(cfg, st) == lib.gsr_capacity_for(ctypes.byref(dims), int(st["num_pairs"] * 1.25) + 4096, int(st["max_list"] * 1.25) + 16)
    # CPU tensors are refused by the compiled path itself
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        be.forward(cfg, torch.zeros(3, 48), torch.zeros(1, 131072, 3), torch.zeros(1, 131072, 6), torch.zeros(1, 131072),
                   torch.zeros(1, 131072, 25, 3), None)
    for small_op in (lambda: be.mark_visible(cfg, torch.zeros(3, 48), torch.zeros(1, 131072, 3)),
                     lambda: be.cov_from_scale_rot(torch.ones(4, 3), torch.ones(4, 4), 1.0),
                     lambda: be.setup_views_backward(torch.zeros(3, 48), torch.zeros(3, 48)),
                     lambda: be.read_status({"bin": torch.zeros(16, dtype=torch.uint8)})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            small_op()
    # the frames of the scale / rotation form are checked before any launch (F = 0 included)
    for frames in (torch.zeros(1, 3, 3, 3), torch.zeros(1, 0, 3, 3), torch.zeros(2, 1, 3, 3)):
        with pytest.raises(ValueError, match="frames must be"):
            ext.frames_arg(cfg, frames)
    fr, nf = ext.frames_arg(cfg, torch.eye(3).expand(1, 2, 3, 3))
    assert nf == 2 and fr.is_contiguous() and ext.frames_arg(cfg, None) == (None, 0)


# ---- the call shape and the dims cross the compiled binding by field: RasterConfig <-> Cfg, _lib.GsrDims <-> GsrDims (no launch, no GPU)
def test_binding_states_the_call_shapes_fields_in_the_dataclasss_order():
    assert _lib.load_torch_ext().CFG_FIELDS == tuple(f.name for f in dataclasses.fields(rasterizer.RasterConfig))


def test_launch_dims_carry_every_field_under_its_own_name():
    """Twelve distinct values in what sizes a call - the eleven fields that reach the dims and the capacity (launch_dims validates
    nothing): a transposed pair anywhere between the dataclass, the binding's table and Cfg::launch_dims shows as a field that is not
    its namesake's."""
    ext = _lib.load_torch_ext()
    flags = _lib.FLAG_SH_IN_FRAME | _lib.FLAG_SH_PLANAR | 0x20  # (an SH-frame bit: launch dims keep it, sizing dims would not)
    cfg = rasterizer.RasterConfig(num_views=11, num_sets=12, views_per_set=13, num_gaussians=14, height=15, width=16, sh_degree=17,
                                  sh_coeffs=18, max_sh_eval=19, has_extra=True, flags=flags, scale_rot=True, alpha=True)
    sizing = [f.name for f in dataclasses.fields(cfg) if f.name not in ("scale_rot", "alpha")]
    cap = (1 << 40) + 21  # (past 32 bits: pair_capacity is the struct's one int64)
    assert len({int(getattr(cfg, n)) for n in sizing} | {cap, _lib.GSR_ABI_VERSION}) == 13  # (has_extra is 1: distinct from the rest)
    dims = ext.launch_dims(cfg, cap)
    assert type(dims) is _lib.GsrDims
    assert [n for n, _ in dims._fields_] == ["abi_version"] + sizing + ["pair_capacity"]
    for name in sizing:
        assert getattr(dims, name) == int(getattr(cfg, name)), name
    assert dims.abi_version == _lib.GSR_ABI_VERSION == 5 and dims.pair_capacity == cap
    assert bytes(rasterizer.HipBackend._dims(cfg, cap)) == bytes(dims)  # callable on the class, the same statement


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("has_extra, scale_rot", [(False, False), (True, False), (False, True), (True, True)])
def test_call_shape_round_trips_through_the_binding(alpha, has_extra, scale_rot):
    """Python -> Cfg (capacity_for's argument conversion) is covered by launch_dims above; Cfg -> Python by prepare_call, whose first
    element is the RasterConfig of the call it was given; and a config read from its attributes comes back equal, bools as bools."""
    ext = _lib.load_torch_ext()
    s, n, m = 2, 8, 9
    cov = torch.zeros(s, n, 7) if scale_rot else torch.zeros(s, n, 6)
    frames = torch.eye(3).expand(s, 2, 3, 3) if scale_rot else None
    got = ext.prepare_call(torch.zeros(s, n, 3), cov, torch.zeros(s, n), torch.zeros(s, n, m, 3), torch.zeros(3 * s, 48), 24, 40, 2, True, 3,
                           torch.zeros(3 * s, n) if has_extra else None, None, 3, False, False, 0, True, False, 1, scale_rot, frames, 1, 0)[0]
    want = rasterizer.RasterConfig(3 * s, s, 3, n, 24, 40, 2, m, 3, has_extra, _lib.FLAG_DEBUG | _lib.FLAG_DETERMINISTIC, scale_rot, False)
    assert type(got) is rasterizer.RasterConfig and got == want
    for cfg in (dataclasses.replace(want, alpha=alpha), dataclasses.replace(want, alpha=alpha, flags=_lib.FLAG_SH_IN_FRAME)):
        back = ext.call_shape(cfg)
        assert type(back) is rasterizer.RasterConfig and back == cfg
        for f in dataclasses.fields(cfg):
            assert type(getattr(back, f.name)) is (bool if f.name in ("has_extra", "scale_rot", "alpha") else int), f.name


def test_binding_refuses_what_is_not_a_call_shape_or_not_dims():
    ext = _lib.load_torch_ext()
    be = rasterizer.HipBackend()
    cfg = rasterizer.RasterConfig(1, 1, 1, 4, 8, 8, 0, 0)
    as_list = [getattr(cfg, f.name) for f in dataclasses.fields(cfg)]
    assert len(as_list) == 13
    for call in (lambda: ext.launch_dims(as_list, 64), lambda: ext.frames_arg(as_list, None),
                 lambda: be._c.capacity_for(as_list, 100, 10, 1.25), lambda: ext.launch_dims(dataclasses.replace(cfg, height=8.0), 64)):
        with pytest.raises(TypeError):
            call()
    t, u8 = torch.zeros(1), torch.zeros(16, dtype=torch.uint8)
    dims = ext.launch_dims(cfg, 64)

    # (dummy CPU tensors: the argument conversion fails, nothing runs)
    for d in (bytes(55), bytes(57), bytes(dims)[:-1], [getattr(dims, n) for n, _ in dims._fields_], None):
        with pytest.raises(TypeError):
            be._c.backward(cfg, d, u8, u8, u8, 0, t, t, t, t, t, None, t, None, False, False, None, 0, None)
