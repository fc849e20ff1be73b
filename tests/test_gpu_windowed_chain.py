"""`-m gpu`: the windowed binning chain (k_preprocess, k_count, k_tile_prefix, k_tile_scan / k_emit<true>, k_emit<false>, contiguous tile
launch; pf3plat_amd/csrc/gsr_hip.hip) on the branches that only large calls reach.  It is an integer pipeline: a lost row group, a
dropped carry or a wrong view offset drops or duplicates list entries.  Each case is held against the CPU oracle for content
(check_preprocess, check_tile_lists on a sample, check_image, check_image_state) and against two exact numpy checks over ALL V x T lists
(tests/parity_checks.py): `ranges_are_the_scan` - the ranges are the exclusive scan of the list lengths, the last end is num_pairs, the
longest list is max_list - and `same_lists_as_fused` - every list equals the fused binning's list of the same call (every case here
has T <= 20 480 tiles, so the fused path takes the same call), with equal num_pairs, max_list and image bits.  Both sides carry
GSR_FLAG_FULL_LISTS, so whole lists are ordered and are compared position by position.

The branches, and the test that names the assertion proving its shape reaches each:
  1. k_tile_prefix, the memory loops of `!in_regs` (more than 512 count-matrix rows)   test_more_than_512_count_matrix_rows_...
  2. k_tile_scan, the second trip of its scan loop and workgroups with c0 >= n            test_more_than_131072_totals_nine_views_...
  3. several views with several 8192-tile windows (k_count, k_emit<false>)                test_more_than_131072_totals_nine_views_...,
                                                                                          test_wide_footprints_across_the_window_boundary_...
  4. the switch V x T <= kEmitScanMax = 8192 between scan-inside-emit and the scan launch test_both_sides_of_the_scan_inside_emit_switch
  5. wide footprints (over the 8 x 8-tile mask window) in the windowed chain              test_wide_footprints_in_scan_inside_emit_...,
                                                                                          test_wide_footprints_across_the_window_boundary_...
  6. overflow on the separate-scan path                                                   test_overflow_on_the_separate_scan_path

Seeds.  Every case's seed was picked on the CPU so that the fp32 oracle in the library's place, held against the fp64 oracle
(`run_oracle(..., oracle_dtype=np.float64)`), passes check_image with NO outlier pixel - the guard of tests/test_general_cameras.py - so
a flipped threshold pixel of the reference cannot be what a failure here means.  To repeat it: `python -m tests.test_gpu_windowed_chain`
(no GPU needed; a minute) prints the guard's figures for every case and fails on a seed that does not meet it.

All cases are forward only except the two of the switch, without harmonics (one colour per Gaussian) and without an extra channel."""
import functools

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, synthetic
from pf3plat_amd.rasterizer import HipBackend, RasterConfig
from tests import gpu_util, parity_checks
from tests.util import look_at_c2w, make_camera, rel_l2

pytestmark = pytest.mark.gpu

WINDOWED = _lib.FLAG_WINDOWED_BINNING | parity_checks.FLAG_FULL_LISTS
FUSED = parity_checks.FLAG_FULL_LISTS
TILE_WINDOW = 8192     # kTileWindow: tiles k_count / k_emit<false> histogram per pass
EMIT_SCAN_MAX = 8192   # kEmitScanMax: most V x T totals k_emit<true> scans itself
FUSED_MAX_TILES = 20480


def _tiles(h, w):
    return 4 * ((h + 15) // 16) * ((w + 15) // 16)


# ------------------------------------------------------------------ the cases' inputs (CPU tensors; a fresh RasterConfig per flag set)
def _cfg(v, n, hw, flags):
    return RasterConfig(v, 1, v, n, hw[0], hw[1], 0, 0, 4, False, flags)


DIM = 0.0125  # largest |colour| of a dimmed scene: one alpha >= 1/255 decision then moves a pixel by at most 2 DIM / 255 = 9.8e-5


def _scene_inputs(seed, n, hw, views, dim=False):
    """synthetic.make_scene's Gaussians and cameras, one colour per Gaussian (its DC coefficient).  dim: colours scaled into [-DIM, DIM]
    (background 0).  check_image's bound is relative to the image norm, so it asks the same of a dim image - but no single threshold
    decision can then make a pixel an outlier (> 1e-4 absolute), and every pixel stays inside the rel-L2 that is asserted.  The two
    large cases need it: with colours of order 1 the fp32 oracle is 14 .. 34 (850 000 Gaussians) and 18 .. 25 (nine views) outlier
    pixels from the fp64 oracle at every one of 30 seeds, so no seed meets the guard."""
    sc = synthetic.make_scene(seed, n, hw, num_views=views, d_sh=1)
    means, cov6, opac, colors = gpu_util.scene_tensors(sc, use_sh=False)
    if dim:
        colors = colors * (DIM / float(colors.abs().max()))
    return gpu_util.scene_viewbuf(sc), means, cov6, opac, colors


def _cov6(rng, s):
    """(n, 3) axis lengths -> (n, 6) covariances under random rotations."""
    n = len(s)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                    2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)
    cov = rot @ (s[:, :, None] ** 2 * np.eye(3)) @ rot.transpose(0, 2, 1)
    return np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], -1)


def _custom_inputs(p, cams):
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))[None]
    vb = gpu_util.viewbuf_from_cams(cams, [(0.2, 0.4, 0.6)] * len(cams))
    return vb, t(p["means"]), t(p["cov6"]), t(p["opac"]), t(p["colors"])


def _wide_700():
    """The scene of test_gpu_parity.test_footprints_wider_than_the_mask_window_deferred_and_inline: 700 splats that each cover 128 x 128."""
    rng = np.random.default_rng(7)
    n = 700
    means = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2, 6, n)], -1)
    cov6 = np.tile([[16.0, 0, 0, 16.0, 0, 16.0]], (n, 1)) * rng.uniform(0.5, 1.5, (n, 1))
    return _custom_inputs(dict(means=means, cov6=cov6, opac=rng.uniform(0.01, 0.05, n), colors=rng.uniform(0, 1, (n, 3))), [make_camera()])


N_ORDINARY, N_WIDE, BOUNDARY_HW = 2000, 300, (1024, 1024)


def _boundary_scene(seeds):
    """Two views of 1024 x 1024: 2 000 ordinary splats (sigma 1 .. 4 px) all over the image, then 300 wide ones (sigma 17 .. 21 px: a radius
    of 3 sigma spans 12 .. 16 tiles) whose centres lie within 30 px of pixel row 512 in view 0.  View 1 turns about the vertical axis
    only, which keeps a point's image row where its depth barely changes.  Pixel of make_camera(): (0.86 x / z + 0.5) * 1024 - 0.5.
    seeds = (ordinary, wide): the two populations are drawn from generators of their own."""
    h, w = BOUNDARY_HW

    def draw(seed, n, row_lo, row_hi, col_margin, z_range, sigma, opacity):
        rng = np.random.default_rng(seed)
        z = rng.uniform(*z_range, n)
        px, py = rng.uniform(col_margin, w - col_margin, n), rng.uniform(row_lo, row_hi, n)
        means = np.stack([((px + 0.5) / w - 0.5) * z / 0.86, ((py + 0.5) / h - 0.5) * z / 0.86, z], -1)
        s = (rng.uniform(*sigma, n) * z / (0.86 * w))[:, None] * rng.uniform(0.8, 1.0, (n, 3))
        return dict(means=means, cov6=_cov6(rng, s), opac=rng.uniform(*opacity, n), colors=rng.uniform(0, 1, (n, 3)))

    a = draw(seeds[0], N_ORDINARY, 0, h, 0, (3.0, 8.0), (1.0, 4.0), (0.2, 0.95))
    b = draw(seeds[1], N_WIDE, 512 - 30, 512 + 30, 0, (4.0, 6.0), (17.0, 21.0), (0.1, 0.25))
    cams = [make_camera(), make_camera(look_at_c2w((0.35, 0.0, 0.0), target=(0, 0, 5.0)))]
    return _custom_inputs({k: np.concatenate([a[k], b[k]]) for k in a}, cams)


# name -> (views, N, (H, W), seed -> inputs, seed).  Seeds: see the module docstring.
CASES = {
    "rows_850k": (1, 850_000, (512, 512), lambda seed: _scene_inputs(seed, 850_000, (512, 512), 1, dim=True), 41),
    "nine_views": (9, 4000, (1024, 1024), lambda seed: _scene_inputs(seed, 4000, (1024, 1024), 9, dim=True), 42),
    "wide_700": (1, 700, (128, 128), lambda seed: _wide_700(), 7),
    "wide_boundary": (2, N_ORDINARY + N_WIDE, BOUNDARY_HW, _boundary_scene, (51, 46)),
    "switch_8192": (2, 3000, (512, 512), lambda seed: _scene_inputs(seed, 3000, (512, 512), 2), 48),
    "switch_8448": (2, 3000, (512, 520), lambda seed: _scene_inputs(seed, 3000, (512, 520), 2), 49),
}


@functools.lru_cache(maxsize=None)
def _inputs(name, seed=None):
    return CASES[name][3](CASES[name][4] if seed is None else seed)


def _cotangent(name):
    v, _, (h, w) = CASES[name][:3]
    return torch.tensor(np.random.default_rng(0).uniform(0, 1, (v, 3, h, w)).astype(np.float32))


def seed_guard(name, seed=None):
    """fp32 oracle in the library's place against the fp64 oracle: check_image with no outlier pixel.  A condition on the seed."""
    v, n, hw = CASES[name][:3]
    cfg = _cfg(v, n, hw, WINDOWED)
    o32, o64 = (gpu_util.run_oracle(cfg, *_inputs(name, seed), oracle_dtype=dt) for dt in (np.float32, np.float64))
    m = parity_checks.check_image(dict(hip=o32, oracle=o64), cfg)
    assert m["outlier_pixels_1e-4"] == 0 and m["color_rel_l2_all"] < parity_checks.TOL, (name, m)
    return m


# ------------------------------------------------------------------ running a case
def _hip_forward(cfg, inputs):
    """The library alone (the fused side of a comparison): -> dict(color, ws)."""
    dev = torch.device("cuda:0")
    be = HipBackend()
    hc, _, _, saved = be.forward(cfg, *(a.to(dev).contiguous() for a in inputs), None)
    torch.cuda.synchronize()
    return dict(color=hc.cpu().numpy(), ws=gpu_util.decode_workspaces(be, cfg, saved), status=be.last_status)


def _rows(cfg):
    """Rows of the count matrix (binning workgroups per view) of a call, from the library's own workspace layout: the counts array
    holds V x rows x (T + 8) entries of 8 bytes (rounded up to 256 bytes, less than a row)."""
    be = HipBackend()
    lay = be.workspace_layout(be._dims(cfg, 1 << 20))
    return (lay["tile_total"] - lay["counts"]) // (cfg.num_views * (_tiles(cfg.height, cfg.width) + 8) * 8)


def _windowed_and_fused(name, g_color=None, lists=True):
    """Run case `name` through the windowed chain (against the oracle) and through the fused binning; both numpy checks over all lists,
    equal image bits.  -> (cfg, res) of the windowed run for the case's own oracle checks."""
    v, n, hw = CASES[name][:3]
    cfg = _cfg(v, n, hw, WINDOWED)
    res = gpu_util.run_both(cfg, *_inputs(name), None, g_color, None)
    ws = res["hip"]["ws"]
    t = _tiles(*hw)
    assert ws["T"] == t <= FUSED_MAX_TILES and ws["depth"] is not None  # (the footprint words are kept only by the windowed chain)
    print(name, "scan", parity_checks.ranges_are_the_scan(ws, v, t))
    fused = _hip_forward(_cfg(v, n, hw, FUSED), _inputs(name))
    assert fused["ws"]["depth"] is None  # the fused binning took that call
    print(name, "lists", parity_checks.same_lists_as_fused(ws, fused["ws"], v, t))
    np.testing.assert_array_equal(res["hip"]["color"], fused["color"])
    return cfg, res


def _content_checks(cfg, res, list_views, max_tiles):
    for v in range(cfg.num_views):
        parity_checks.check_preprocess(res, cfg, v)
        parity_checks.check_image_state(res, cfg, v)
    for v in list_views:
        m = parity_checks.check_tile_lists(res, cfg, v, max_tiles=max_tiles)
        assert m["prefix_only_tiles"] == 0, m
    return parity_checks.check_image(res, cfg)


# ------------------------------------------------------------------ the tests
def test_more_than_512_count_matrix_rows_take_the_memory_loops_of_k_tile_prefix():
    """Branch 1: k_tile_prefix keeps a thread's rows in registers only while rpg = ceil(R / 64) <= kPrefixRegs = 8, i.e. R <= 512 rows;
    850 000 Gaussians at 512 x 512 have more (asserted from the workspace layout, and from N > 512 x kChunkPrefer), so both memory
    loops (`for (int r = r0; r < r1; ++r)`: the sum, and the write-back of the running prefix) carry every list's offsets."""
    name = "rows_850k"
    v, n, hw = CASES[name][:3]
    # choose_chunk never picks more than kChunkPrefer = 1600 Gaussians per row, so R >= N / 1600 > 512 = 64 x kPrefixRegs: `!in_regs`
    assert n > 512 * 1600
    assert _rows(_cfg(v, n, hw, WINDOWED)) > 512
    cfg, res = _windowed_and_fused(name)
    _content_checks(cfg, res, [0], max_tiles=48)
    assert res["hip"]["status"]["num_pairs"] > 2_500_000


def test_more_than_131072_totals_nine_views_of_two_windows_each():
    """Branches 2 and 3: 9 views of 1024 x 1024 are V x T = 147 456 totals.  tile_scan_blocks caps k_tile_scan at 128 workgroups, so its
    chunk is 2048: `for (s0 = c0; s0 < c1; s0 += 1024)` takes two trips and `carry += step` carries the first into the second, and the
    workgroups from 72 on start at c0 >= n.  T = 16 384 is two 8192-tile windows, so k_count and k_emit<false> offset by
    (v * rows + row) * T and ranges + v * T inside their window loops for nine views."""
    name = "nine_views"
    v, n, hw = CASES[name][:3]
    t = _tiles(*hw)
    assert v * t == 147_456 > 128 * 1024 and t == 2 * TILE_WINDOW
    chunk = ((v * t + 127) // 128 + 1023) // 1024 * 1024  # k_tile_scan's chunk with gridDim.x = 128
    assert chunk == 2048 and 127 * chunk >= v * t  # two trips; trailing workgroups have nothing
    cfg, res = _windowed_and_fused(name)
    _content_checks(cfg, res, [0, 4, 8], max_tiles=64)
    assert rel_l2(res["hip"]["color"][0], res["hip"]["color"][8]) > 1e-2  # (a kernel that read one view's rows for all would show)
    assert rel_l2(res["oracle"]["color"][0], res["oracle"]["color"][8]) > 1e-2


def test_wide_footprints_in_scan_inside_emit_deferred_list_and_inline_walk():
    """Branch 5, in k_emit<true>: 700 splats that each cover all 16 x 16 tiles of a 128 x 128 image (wider than the 8 x 8-tile mask
    window) in at most two binning workgroups: the deferred list `bigs[kBigList = 256]` of the first fills and its other footprints are walked in line."""
    name = "wide_700"
    v, n, hw = CASES[name][:3]
    assert v * _tiles(*hw) <= EMIT_SCAN_MAX and n > 256 * _rows(_cfg(v, n, hw, WINDOWED))  # a workgroup with more than kBigList of them
    cfg, res = _windowed_and_fused(name)
    assert res["hip"]["status"]["max_list"] >= 600
    assert (res["oracle"]["radii"][0] >= 64).sum() >= 600  # footprints over the whole 128 x 128 image: 16 x 16 tiles
    _content_checks(cfg, res, [0], max_tiles=64)


def test_wide_footprints_across_the_window_boundary_in_two_views():
    """Branches 5 and 3, in k_count / k_emit<false>: for_each_pair walks a wide footprint with big_walk_lane and keeps the tiles with
    t0 <= t < t1.  Two views of 1024 x 1024 (T = 16 384: tile row 64, tile index 8192, starts the second window); 300 splats span at
    least 12 x 12 tiles around pixel row 512, so each belongs to both windows.  Every tile of tile rows 62 .. 66 is checked."""
    name = "wide_boundary"
    v, n, hw = CASES[name][:3]
    t = _tiles(*hw)
    sgx = 2 * ((hw[1] + 15) // 16)
    assert t == 2 * TILE_WINDOW and 64 * sgx == TILE_WINDOW and v * t > EMIT_SCAN_MAX
    cfg, res = _windowed_and_fused(name)
    for view in range(v):
        geo = res["oracle"]["handles"][view][0].geometry()
        xy, rad = geo["xy"][N_ORDINARY:], res["oracle"]["radii"][view][N_ORDINARY:].astype(np.float64)
        wide = (2 * rad >= 12 * 8) & (xy[:, 0] - rad >= 0) & (xy[:, 0] + rad <= hw[1] - 1)  # >= 12 x 12 tiles, all inside the image
        near = np.abs(xy[:, 1] - 512) <= 40
        crosses = (np.floor((xy[:, 1] - 0.5 * rad) / 8) <= 63) & (np.floor((xy[:, 1] + 0.5 * rad) / 8) >= 64)  # (well inside the radius)
        assert (wide & near & crosses).sum() >= 100, (view, int(wide.sum()), int(near.sum()), int(crosses.sum()))
        # and some reach tile 8191 itself, the LAST tile of the first window (tile row 63, column 127: pixels from 1016, rows 504 .. 511)
        last = (2 * rad >= 12 * 8) & (xy[:, 0] + 0.5 * rad >= 1016) & (xy[:, 0] <= 1023) & (np.abs(xy[:, 1] - 508) <= 0.5 * rad)
        assert last.sum() >= 3, (view, int(last.sum()))
    _content_checks(cfg, res, [], max_tiles=None)
    rows = np.arange(62 * sgx, 67 * sgx)
    for view in range(v):
        m = parity_checks.check_tile_lists(res, cfg, view, tiles=rows)
        assert m["checked_tiles"] == 5 * sgx and m["pairs"] > 20 * sgx and m["prefix_only_tiles"] == 0, m


@pytest.mark.parametrize("name, vt, scan_in_emit", [("switch_8192", 8192, True), ("switch_8448", 8448, False)])
def test_both_sides_of_the_scan_inside_emit_switch(name, vt, scan_in_emit):
    """Branch 4: `scan_in_emit = V x T <= kEmitScanMax`.  Two views of 512 x 512 are exactly 8192 totals: k_emit<true> with all eight
    totals per thread, and for view 1 `lo_t = T = 4096`: half of every workgroup's threads hold the cursors.  Two views of 512 x 520 are
    2 x 4224 = 8448: k_tile_scan with nine workgroups, the last one with 256 of its 1024 totals, then k_emit<false> over one window.
    Forward and backward, all checks."""
    v, n, hw = CASES[name][:3]
    t = _tiles(*hw)
    assert v * t == vt and (vt <= EMIT_SCAN_MAX) == scan_in_emit and t <= TILE_WINDOW
    if scan_in_emit:
        assert -(-vt // 1024) == 8  # `per`: totals per thread of k_emit<true>
    else:
        assert -(-vt // 1024) == 9 and vt - 8 * 1024 == 256  # k_tile_scan: nine workgroups of 1024, the last partial
    cfg, res = _windowed_and_fused(name, g_color=_cotangent(name))
    parity_checks.all_checks(cfg, res, max_tiles=256)


def test_overflow_on_the_separate_scan_path():
    """Branch 6: the 8448-total case with a pair workspace that is too small.  k_tile_scan then writes (0, 0) for every range and the
    flag, k_emit<false> returns on `status->overflow`, the tile launch poisons the image.  Through the operator (`capacity=100`) the
    retry gives the uncapped run's image bit for bit; through the plan API the refused attempt itself is read."""
    name = "switch_8448"
    v, n, hw = CASES[name][:3]
    t = _tiles(*hw)
    assert v * t == 8448 > EMIT_SCAN_MAX
    cfg = _cfg(v, n, hw, WINDOWED)
    free = _hip_forward(cfg, _inputs(name))
    true_pairs = free["ws"]["num_pairs"]
    assert free["status"]["overflow"] == 0 and true_pairs > 1000
    res = gpu_util.run_both(cfg, *_inputs(name), capacity=100)
    assert res["hip"]["status"]["overflow"] == 0 and res["hip"]["status"]["num_pairs"] == true_pairs
    np.testing.assert_array_equal(res["hip"]["color"], free["color"])
    parity_checks.check_image(res, cfg)
    parity_checks.ranges_are_the_scan(res["hip"]["ws"], v, t)
    # the refused attempt
    dev = torch.device("cuda:0")
    be = HipBackend()
    plan = be.make_plan(cfg, dev, capacity=true_pairs // 2)
    be.bind_forward(plan, *(a.to(dev).contiguous() for a in _inputs(name)))()
    st = be.read_status(plan)
    torch.cuda.synchronize()
    assert st["overflow"] == 1 and st["num_pairs"] == true_pairs, st
    lay = be.workspace_layout(plan["dims"])
    ranges = plan["bin"][lay["ranges"]: lay["ranges"] + v * t * 8].view(torch.int32).cpu().numpy()
    assert ranges.shape == (2 * v * t,) and not ranges.any()  # every decoded range is (0, 0)
    assert bool(torch.isnan(plan["color"]).all())  # and the image says so to a caller who reads no status


if __name__ == "__main__":
    for case_name in CASES:
        print(case_name, seed_guard(case_name))
