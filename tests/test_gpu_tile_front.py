"""`-m gpu`: the front of the forward tile launch k_tile_fwd_prefix (pf3plat_amd/csrc/gsr_tiles_fwd.h) - what a tile does before its
first blend.  Two things there depend on sizes a random scene rarely puts on their edges:
  * a thread copies its binning row's run for the tile GSR_RUN_STEP (18) keys per step, all loads of a step requested together;
    runs of more than 24 keys go to the cooperative long-run path;
  * the rank pass hands the first batches to the blend through LDS (the ids of list positions < 320, the records of batches 0 and
    1, null records from the list's end on) and the blend's first pass enters through the primed prologue; n == 1, the bitonic
    fallback, the general path and the second pass of a tile still open behind its ranked prefix take the ordinary prologue.
The yardstick is in the tree: the plan's pair capacity selects the tile kernel (slot = capacity / (2 x tiles): <= 640 and > 2048 give
the two k_tile_fwd instances, which know none of this), and every kernel blends with the same arithmetic in the same order.  Every
case renders one call through k_tile_fwd_prefix (slot 1024) and through k_tile_fwd<., 4096> (slot 2100) and compares colour,
final_T, n_contrib, radii, list lengths, walked counts and walked list prefixes with torch.equal.

The placed scenes are built on the CPU: camera 0 of synthetic.make_scene sits at the origin and looks down +z with focal length
0.86 x the image side, so a Gaussian at depth d on the ray through a tile's centre, 0.3 pixels wide, is listed by that tile alone
whatever its opacity (its footprint ends 2.6 pixels from the centre at most); Gaussians nobody places sit behind the camera.  Consecutive
indices inside one binning chunk (512 Gaussians for these calls) on one tile are one run of the pair matrix.  Each test asserts from
the call's own lists and pair matrix that the sizes it is about occurred."""
import functools

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, synthetic
from pf3plat_amd.rasterizer import RasterConfig
from tests import gpu_util, parity_checks
from tests.test_gpu_tile_deal import _assert_same, _Call, _dev, _gpu

pytestmark = pytest.mark.gpu

HW, SG, T = (128, 128), 16, 256  # 16 x 16 tiles of 8 x 8 pixels
FOCAL = 0.86  # synthetic.make_scene
CHUNK = 512  # Gaussians per binning row for one view of up to 8 192 Gaussians (gsr_common.h choose_chunk: one round of the smallest chunk)
SLOT_PREFIX, SLOT_WIDE = 1024, 2100
RUNS = (1, 6, 7, 12, 13, 18, 19, 24, 25)  # the copy's steps of 6 (the 80-register instances), 12, 18, 24 keys; 25: the long-run path
LENS = (2, 31, 32, 33, 63, 64, 65, 319, 320, 321, 640, 641)  # batches 0 / 1, the handed-over ids' end, where the prefix rank begins


def _tile(k):
    """The k-th target tile: odd tile coordinates, so that no two targets are neighbours."""
    return (1 + 2 * (k // 8)) * SG + 1 + 2 * (k % 8)


@functools.lru_cache(maxsize=None)
def _placed(n_total, groups, seed=21):
    """groups: ((tile, first index, count, opacity, one_depth), ...) -> (viewbuf, means, cov6, opac, colors) on the CPU.  A group's
    Gaussians sit on the ray through their tile's centre at depths 2 ... 5 (one_depth: all at 3 - one depth bucket)."""
    sc = synthetic.make_scene(seed, n_total, HW)
    means, cov6, opac, colors = (t.clone() for t in gpu_util.scene_tensors(sc))
    means[0] = torch.tensor([0.0, 0.0, -5.0])
    for tile, first, count, opacity, one_depth in groups:
        d = torch.full((count,), 3.0) if one_depth else torch.linspace(2.0, 5.0, count)
        _put(means, cov6, opac, HW, (tile % SG, tile // SG), slice(first, first + count), d, 0.3, opacity)
    return gpu_util.scene_viewbuf(sc), means, cov6, opac, colors


def _put(means, cov6, opac, hw, tile_xy, sl, d, sigma_px, opacity):
    """Gaussians `sl` onto the ray of camera 0 through the centre of tile (x, y) at depths d, sigma_px pixels wide (square images)."""
    cx, cy = 8 * tile_xy[0] + 4, 8 * tile_xy[1] + 4  # pixel coordinate + 0.5 of the tile's centre
    ray = torch.tensor([(cx / hw[1] - 0.5) / FOCAL, (cy / hw[0] - 0.5) / FOCAL, 1.0])
    means[0, sl] = d[:, None] * ray
    s2 = (sigma_px / (FOCAL * hw[1]) * d) ** 2
    cov6[0, sl] = torch.stack((s2, 0 * s2, 0 * s2, s2, 0 * s2, s2), -1)
    opac[0, sl] = opacity


def _scene_a():
    """Nine tiles whose list is one run of RUNS[r] keys from binning row r; twelve tiles listing LENS[k] entries."""
    groups = [(_tile(r), CHUNK * r, ln, 0.3, False) for r, ln in enumerate(RUNS)]
    first = CHUNK * len(RUNS)
    for k, ln in enumerate(LENS):
        groups.append((_tile(len(RUNS) + k), first, ln, 0.3, False))
        first += ln
    assert first <= 8000
    return tuple(groups)


FAINT, ONE_DEPTH, LONG = 760, 60, 1100


def _scene_b():
    """A tile of 760 faint entries (opacity 0.02: nothing stops, the blend comes back for the rest of the list behind the ranked
    prefix); 60 entries at one depth (more than kSpanMax = 48 in a bucket: the bitonic fallback); 1100 entries (longer than the slot
    of 1024: the general path, its list in the tail pool); one entry."""
    return ((_tile(0), 0, FAINT, 0.02, False), (_tile(1), 768, ONE_DEPTH, 0.3, True), (_tile(2), 832, LONG, 0.02, False),
            (_tile(3), 1935, 1, 0.3, False))


def _expected(groups):
    want = np.zeros(T, dtype=np.int64)
    for tile, _, count, _, _ in groups:
        want[tile] += count
    return want


def _forward(cfg, slot, ins_cpu, backward=False):
    """One forward of `cfg` on the tile kernel that `slot` selects -> (_Call, what test_gpu_tile_deal's _Call.forward returns, plus
    the extra / alpha images)."""
    call = _Call(cfg, 2 * cfg.num_views * T_of(cfg) * slot, backward=backward)
    assert int(call.plan["dims"].pair_capacity) // (2 * call.VT) == slot
    out = call.forward(_gpu(ins_cpu))
    assert not torch.isnan(out["color"]).any()
    for k in ("extra_img", "alpha_img"):
        out[k] = None if call.plan[k] is None else call.plan[k].cpu().clone()
    return call, out


def T_of(cfg):
    return 4 * ((cfg.height + 15) // 16) * ((cfg.width + 15) // 16)


def _same(a, b, what):
    _assert_same(a, b, what)
    for k in ("extra_img", "alpha_img"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), (what, k)
    for k in ("overflow", "max_list", "num_pairs"):
        assert a["status"][k] == b["status"][k], (what, k)


@functools.lru_cache(maxsize=None)
def _both(n_total, groups, flags=0):
    """The placed scene through both kernels -> (prefix call, prefix outputs, k_tile_fwd<., 4096> outputs); compared here, once."""
    assert 640 < SLOT_PREFIX <= 2048 < SLOT_WIDE  # k_tile_fwd_prefix | k_tile_fwd<., 4096>
    cfg = RasterConfig(1, 1, 1, n_total, HW[0], HW[1], 4, 25, 4, False, flags)
    ins = _placed(n_total, groups)
    call, front = _forward(cfg, SLOT_PREFIX, ins)
    _, wide = _forward(cfg, SLOT_WIDE, ins)
    _same(wide, front, "prefix against k_tile_fwd<4096>")
    assert np.array_equal(front["list_len"].numpy(), _expected(groups))  # the scene is what the test is about
    return call, front, wide


def _pair_matrix(call, n_total):
    """-> (rows, T) run lengths of the call's pair matrix (csrc: pair_mat[(view x rows + row) x (T + 8) + tile] = (offset, count))."""
    rows = -(-n_total // CHUNK)
    lay = call.lay["counts"]
    m = call.plan["bin"][lay: lay + rows * (T + 8) * 8].view(torch.int32).reshape(rows, T + 8, 2)[:, :T, 1].cpu().numpy().astype(np.int64)
    return m


def test_run_lengths_at_the_edges_of_the_copy_steps():
    """Runs of 1, 6, 7, 12, 13, 18, 19, 24 keys (the short-run copy at every step size it has had or may be built with) and 25 (the
    long-run path), each the whole list of its tile; the longer lists of the scene are runs of up to 512 keys."""
    call, front, _ = _both(8000, _scene_a())
    m = _pair_matrix(call, 8000)
    assert np.array_equal(m.sum(0), front["list_len"].numpy())  # the matrix was decoded with the call's rows
    for r, ln in enumerate(RUNS):
        assert m[r, _tile(r)] == ln and (m[:, _tile(r)] != 0).sum() == 1, (r, ln, m[:, _tile(r)])
    assert m.max() > 320  # the long-run path with a run many descriptors' worth of keys
    assert torch.equal(front["walked"], front["list_len"])  # nothing stops: every key that was copied is blended


def test_list_lengths_at_the_edges_of_the_hand_over():
    """n = 2, 31 ... 33, 63 ... 65 (null records inside batches 0 and 1), 319 ... 321 (the end of the handed-over ids), 640 / 641
    (where the prefix rank begins) and n = 1 (no rank pass: the ordinary prologue): bits as k_tile_fwd<., 4096>'s, all entries walked."""
    _, front, _ = _both(8000, _scene_a())
    for k, ln in enumerate(LENS):
        t = _tile(len(RUNS) + k)
        assert int(front["list_len"][t]) == ln and int(front["walked"][t]) == ln, (ln, t)
    assert int(front["list_len"][_tile(0)]) == 1 and int(front["walked"][_tile(0)]) == 1
    assert int(front["n_contrib"].max()) == max(LENS)  # the pixel at a tile's centre blends its whole list


def test_the_whole_list_ranked_at_once():
    """GSR_FLAG_FULL_LISTS: ranked = n for every list - the 641-entry tile hands over too, and its whole list is in depth order."""
    call, front, wide = _both(8000, _scene_a(), _lib.FLAG_FULL_LISTS)
    t = _tile(len(RUNS) + LENS.index(641))
    a = int(front["range_start"][t])
    ids = call.words("point_list", int(call.plan["dims"].pair_capacity)).cpu()[a: a + 641].numpy()
    first = CHUNK * len(RUNS) + sum(LENS[:-1])
    assert np.array_equal(ids, np.arange(first, first + 641))  # depths rise with the index


def test_oracle_parity_of_the_placed_scene():
    cfg = RasterConfig(1, 1, 1, 8000, HW[0], HW[1], 4, 25, 4, False)
    call, front, _ = _both(8000, _scene_a())
    saved = (call.plan["dims"], call.plan["geom"], call.plan["bin"], call.plan["img"])
    res = dict(hip=dict(color=front["color"].numpy(), extra=None, radii=front["radii"].numpy(),
                        ws=gpu_util.decode_workspaces(call.be, cfg, saved), status=front["status"]),
               oracle=gpu_util.run_oracle(cfg, *_placed(8000, _scene_a())))
    parity_checks.all_checks(cfg, res, max_tiles=None)


def test_a_tile_still_open_behind_its_ranked_prefix():
    """760 faint entries: the first pass (primed) ends with every pixel open, the rest is ranked and the second pass (b0 > 0) takes
    the ordinary prologue."""
    _, front, _ = _both(2048, _scene_b())
    assert int(front["list_len"][_tile(0)]) == FAINT > 640 and int(front["walked"][_tile(0)]) == FAINT


def test_the_paths_that_keep_the_ordinary_prologue():
    """One entry; 60 keys in one depth bucket (the bitonic fallback); a list longer than its slot (the general path)."""
    _, front, wide = _both(2048, _scene_b())
    for k, ln in ((1, ONE_DEPTH), (2, LONG), (3, 1)):
        assert int(front["list_len"][_tile(k)]) == ln and int(front["walked"][_tile(k)]) == ln, (k, ln)
    assert int(front["range_start"][_tile(2)]) >= T * SLOT_PREFIX  # in the tail pool: sort_tile_general_2048 took it
    assert int(wide["range_start"][_tile(2)]) < T * SLOT_WIDE  # and k_tile_fwd<., 4096> had it in its slot


@pytest.mark.parametrize("what", ["extra", "alpha", "three_views"])
def test_the_other_instances_on_drawn_scenes(what):
    """The extra channel (kExtra), the accumulated alpha (kAlpha), three views of 64 x 64 in one call (the instance built for four waves
    per SIMD over several views) on independently drawn scenes - lists of every length up to ~190 - with 300 opaque Gaussians six
    pixels wide in front of one tile: that tile and its neighbours stop after their first batches."""
    views, hw, n = (3, (64, 64), 4000) if what == "three_views" else (1, HW, 8000)
    sc = synthetic.make_scene(22, n, hw, num_views=views)
    means, cov6, opac, colors = (t.clone() for t in gpu_util.scene_tensors(sc))
    _put(means, cov6, opac, hw, (3, 3), slice(0, 300), torch.linspace(1.2, 1.5, 300), 6.0, 0.9)
    ins = (gpu_util.scene_viewbuf(sc), means, cov6, opac, colors)
    if what == "extra":
        ins += (torch.rand((1, n), generator=torch.Generator().manual_seed(1)) + 0.5,)
    cfg = RasterConfig(views, 1, views, n, hw[0], hw[1], 4, 25, 4, what == "extra", 0, False, what == "alpha")
    _, front = _forward(cfg, SLOT_PREFIX, ins)
    _, wide = _forward(cfg, SLOT_WIDE, ins)
    _same(wide, front, what)
    assert (front["extra_img"] is not None) == (what == "extra") and (front["alpha_img"] is not None) == (what == "alpha")
    assert int(front["list_len"].max()) > 64 and int((front["walked"] < front["list_len"]).sum()) > 0
    assert front["status"]["max_list"] <= SLOT_PREFIX  # every tile on the bucketed path's side of the slot


def test_the_backward_does_not_depend_on_the_forward_instance():
    """FLAG_BACKWARD_FOLLOWS | FLAG_DETERMINISTIC, forward + backward: equal gradients whichever tile kernel ran the forward."""
    flags = _lib.FLAG_BACKWARD_FOLLOWS | _lib.FLAG_DETERMINISTIC
    n = 8000
    sc = synthetic.make_scene(23, n, HW)
    ins = (gpu_util.scene_viewbuf(sc),) + tuple(gpu_util.scene_tensors(sc))
    cfg = RasterConfig(1, 1, 1, n, HW[0], HW[1], 4, 25, 4, False, flags)
    g_color = torch.rand((1, 3) + HW, generator=torch.Generator().manual_seed(3)).to(_dev())
    grads, outs = [], []
    for slot in (SLOT_PREFIX, SLOT_WIDE):
        call, out = _forward(cfg, slot, ins, backward=True)
        call.be.run_backward(call.plan, *_gpu(ins), None, g_color)
        torch.cuda.synchronize()
        outs.append(out)
        grads.append({k: call.plan[k].cpu().clone() for k in ("d_means", "d_cov6", "d_opac", "d_colors", "d_means2d")})
    _same(outs[1], outs[0], "forward")
    for k, g in grads[0].items():
        assert torch.isfinite(g).all() and bool((g != 0).any()), k
        assert torch.equal(g, grads[1][k]), k
