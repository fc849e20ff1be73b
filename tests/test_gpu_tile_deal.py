"""`-m gpu`: the forward tile launch's deal (pf3plat_amd/csrc/gsr_common.h: build_tile_order, fwd_tile_of).  One view whose tiles fill
no more than the first resident round takes its tile -> workgroup order from a table (`tile_order` in the `bin` workspace) that the
binning launch builds from the walked counts (`tile_total`) the plan's PREVIOUS forward left: an XCD's tiles dealt to its compute
units heaviest first, every other round of 32 mirrored - k_blend_bwd's order.  Whatever the counts hold, placement must be a
permutation of the tiles and must not touch a bit of the results.

Shapes: 256 x 256 (1024 tiles: the smallest image that fills the round) and 30 000 Gaussians (~120 entries per tile).  The plan's pair
capacity selects the tile kernel: slot = capacity / (2 x tiles); <= 640 -> k_tile_fwd<true, 2048>, 641 ... 2048 -> k_tile_fwd_prefix.
Every comparison is exact (torch.equal); the oracle parity helpers run once, on the prefix instance under the descending hint."""
import functools

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, synthetic
from pf3plat_amd.rasterizer import HipBackend, RasterConfig
from tests import gpu_util, parity_checks

pytestmark = pytest.mark.gpu

N, HW, T = 30000, (256, 256), 1024
SLOTS = {"k_tile_fwd": 512, "k_tile_fwd_prefix": 1024}
HINTS = ("zeros", "ones", "equal", "ascending", "descending", "random", "previous", "other_scene")
SENTINEL = 0x5EEDF00D  # never a tile number


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _scene(seed, n=N, hw=HW, views=1):
    """-> (viewbuf, means, cov6, opac, colors) on the CPU; the viewbuf by the oracle's camera arithmetic (both sides render with it)."""
    sc = synthetic.make_scene(seed, n, hw, num_views=views)
    return (gpu_util.scene_viewbuf(sc),) + tuple(gpu_util.scene_tensors(sc))


def _gpu(ins):
    return tuple(t.to(_dev()).contiguous() for t in ins)


@functools.lru_cache(maxsize=None)
def _dense_scene():
    """Scene 11 with its first 1500 Gaussians moved onto one visible Gaussian near the image centre (small, faint): that tile lists
    more than 1024 entries - longer than its slot, so its list goes to the tail pool and through sort_tile's general path."""
    vb, means, cov6, opac, colors = _scene(11)
    be = HipBackend()
    cfg = RasterConfig(1, 1, 1, N, HW[0], HW[1], 4, 25, 4, False)
    plan = be.make_plan(cfg, _dev(), capacity=2 * T * 1024)
    be.run_forward(plan, *_gpu((vb, means, cov6, opac, colors)))
    torch.cuda.synchronize()
    xy = plan["geom"][: N * 32].view(torch.float32).reshape(N, 8)[:, :2].cpu().numpy()
    vis = plan["radii"].reshape(-1).cpu().numpy() > 0
    d = np.where(vis, np.abs(xy[:, 0] - 131.5) + np.abs(xy[:, 1] - 123.5), np.inf)  # the middle of tile (16, 15)
    g0 = int(np.argmin(d))
    assert d[g0] < 3.0, d[g0]
    means, cov6, opac = means.clone(), cov6.clone(), opac.clone()
    k = 1500
    rows = torch.arange(N) != g0
    rows = torch.nonzero(rows)[:k, 0]
    means[0, rows] = means[0, g0].clone()
    cov6[0, rows] = cov6[0, g0].clone() * 0.05
    opac[0, rows] = 0.02
    return (vb, means, cov6, opac, colors), (int(xy[g0, 1]) // 8) * 32 + int(xy[g0, 0]) // 8


def _xcd_ranges(tiles):
    """-> [(first tile, count)] of the eight XCDs (xcd_remap: workgroup b runs on XCD b % 8 and XCD x owns a contiguous run)."""
    q, r = tiles >> 3, tiles & 7
    return [((x * (q + 1) if x < r else r * (q + 1) + (x - r) * q), q + (1 if x < r else 0)) for x in range(8)]


def _expected_order(hint, tiles):
    """The table the issue defines, from the hint alone: per XCD the keys (min(count, 0xfffffe) + 1) << 8 | (255 - index), descending;
    the XCD's k-th workgroup (block 8 k + xcd) takes position (k >> 5) << 5 | in, `in` mirrored inside odd rounds."""
    out = np.zeros(tiles, dtype=np.int64)
    for x, (base, cnt) in enumerate(_xcd_ranges(tiles)):
        c = hint[base: base + cnt].astype(np.int64) & 0xFFFFFFFF
        keys = ((np.minimum(c, 0xFFFFFE) + 1) << 8) | (255 - np.arange(cnt))
        by_load = np.argsort(-keys, kind="stable")
        for k in range(cnt):
            rnd, j = k >> 5, k & 31
            ln = min(32, cnt - (rnd << 5))
            out[8 * k + x] = base + by_load[(rnd << 5) + (ln - 1 - j if rnd & 1 else j)]
    return out


class _Call:
    """One plan of the shape under test and the means to run it under a hint."""

    def __init__(self, cfg, capacity, backward=False):
        self.be, self.cfg = HipBackend(), cfg
        self.plan = self.be.make_plan(cfg, _dev(), capacity=capacity, backward=backward)
        self.lay = self.be.workspace_layout(self.plan["dims"])
        self.VT = cfg.num_views * 4 * ((cfg.height + 15) // 16) * ((cfg.width + 15) // 16)

    def words(self, name, count=None):
        count = self.VT if count is None else count
        return self.plan["bin"][self.lay[name]: self.lay[name] + 4 * count].view(torch.int32)

    def hint_words(self, kind, ins_gpu, other_gpu=None):
        """Leaves `kind` in tile_total; -> what it left (int64 numpy, as unsigned)."""
        tt, n = self.words("tile_total"), self.VT
        g = torch.Generator().manual_seed(5)
        if kind == "previous":
            self.be.run_forward(self.plan, *ins_gpu)
        elif kind == "other_scene":
            self.be.run_forward(self.plan, *other_gpu)
        else:
            pat = {"zeros": torch.zeros(n, dtype=torch.int64), "ones": torch.full((n,), 0xFFFFFFFF, dtype=torch.int64),
                   "equal": torch.full((n,), 7, dtype=torch.int64), "ascending": torch.arange(n, dtype=torch.int64),
                   "descending": n - 1 - torch.arange(n, dtype=torch.int64),
                   "random": torch.randint(0, 1 << 20, (n,), generator=g, dtype=torch.int64)}[kind]
            tt.copy_(pat.to(torch.int32) if kind != "ones" else torch.full((n,), -1, dtype=torch.int32))
        torch.cuda.synchronize()
        return tt.cpu().numpy().astype(np.int64) & 0xFFFFFFFF

    def forward(self, ins_gpu):
        """NaN in the image first; -> dict of CPU tensors: everything the call returns or leaves for its backward."""
        p = self.plan
        p["color"].fill_(float("nan"))
        self.words("tile_order").fill_(SENTINEL)
        self.be.run_forward(p, *ins_gpu)
        st = self.be.read_status(p)
        assert st["overflow"] == 0, st
        V, H, W = self.cfg.num_views, self.cfg.height, self.cfg.width
        rg = self.plan["bin"][self.lay["ranges"]: self.lay["ranges"] + 8 * self.VT].view(torch.int32).reshape(self.VT, 2).cpu()
        walked = self.words("tile_total").cpu()
        plist = self.words("point_list", int(p["dims"].pair_capacity)).cpu()
        # every tile's list up to what its blend walked, laid end to end (a list's PLACE in the tail pool is first come, first served)
        idx = torch.cat([torch.arange(int(a), int(a) + min(int(w), int(b - a))) for (a, b), w in zip(rg.tolist(), walked.tolist())])
        img = p["img"]
        return dict(color=p["color"].cpu().clone(), radii=p["radii"].cpu().clone(),
                    final_T=img[self.lay["final_T"]: self.lay["final_T"] + 4 * V * H * W].view(torch.int32).cpu().clone(),
                    n_contrib=img[self.lay["n_contrib"]: self.lay["n_contrib"] + 4 * V * H * W].view(torch.int32).cpu().clone(),
                    list_len=(rg[:, 1] - rg[:, 0]).clone(), walked=walked.clone(), lists=plist[idx].clone(), range_start=rg[:, 0].clone(),
                    order=self.words("tile_order").cpu().numpy().astype(np.int64) & 0xFFFFFFFF, status=st)


def _assert_same(a, b, what):
    for k in ("color", "radii", "final_T", "n_contrib", "list_len", "walked", "lists"):
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("kernel", sorted(SLOTS))
def test_bits_do_not_depend_on_the_hint_and_every_tile_is_taken_once(kernel):
    """All eight hints: the same colour, final_T, n_contrib, radii, list lengths and walked list prefixes; no NaN left in the image;
    tile_order is the permutation the hint defines, every tile on its xcd_remap XCD.  The descending hint's call of the prefix instance
    also goes through the oracle parity helpers."""
    cfg = RasterConfig(1, 1, 1, N, HW[0], HW[1], 4, 25, 4, False)
    call = _Call(cfg, 2 * T * SLOTS[kernel])
    assert int(call.plan["dims"].pair_capacity) // (2 * T) == SLOTS[kernel]
    scene, other = _scene(11), _gpu(_scene(12))
    ins = _gpu(scene)
    first = None
    for kind in HINTS:
        hint = call.hint_words(kind, ins, other)
        out = call.forward(ins)
        assert not torch.isnan(out["color"]).any(), kind
        order = out["order"]
        assert np.array_equal(np.sort(order), np.arange(T)), kind  # a permutation
        for x, (base, cnt) in enumerate(_xcd_ranges(T)):
            mine = order[x::8]
            assert len(mine) == cnt and mine.min() >= base and mine.max() < base + cnt, (kind, x)  # on its own XCD
        assert np.array_equal(order, _expected_order(hint, T)), kind
        if kind in ("zeros", "ones", "equal"):  # equal loads: index order, mirrored in odd rounds - not the identity
            assert not np.array_equal(order, np.array([_xcd_ranges(T)[b & 7][0] + (b >> 3) for b in range(T)]))
        if first is None:
            first = out
        _assert_same(first, out, kind)
        if kind == "descending" and kernel == "k_tile_fwd_prefix":
            saved = (call.plan["dims"], call.plan["geom"], call.plan["bin"], call.plan["img"])
            res = dict(hip=dict(color=out["color"].numpy(), extra=None, radii=out["radii"].numpy(),
                                ws=gpu_util.decode_workspaces(call.be, cfg, saved), status=out["status"]),
                       oracle=gpu_util.run_oracle(cfg, *scene))
            parity_checks.all_checks(cfg, res, max_tiles=48)
    assert int(first["walked"].max()) > int(first["walked"].min())  # the "previous" hint was a real load profile


@pytest.mark.parametrize("kernel", sorted(SLOTS))
def test_the_general_path_renders_the_dealt_tile(kernel):
    """One tile lists more than its slot holds (n > stride: sort_tile_general_2048 / sort_tile's tail-pool branch), and the hints put
    that tile on another workgroup than image order does: the image equals the all-equal hint's."""
    cfg = RasterConfig(1, 1, 1, N, HW[0], HW[1], 4, 25, 4, False)
    call = _Call(cfg, 2 * T * SLOTS[kernel])
    scene, dense_tile = _dense_scene()
    ins = _gpu(scene)
    outs = {}
    for kind in ("equal", "descending", "random"):
        call.hint_words(kind, ins)
        outs[kind] = out = call.forward(ins)
        assert not torch.isnan(out["color"]).any(), kind
        assert out["status"]["max_list"] >= int(out["list_len"][dense_tile]) > SLOTS[kernel]
        assert int(out["range_start"][dense_tile]) >= T * SLOTS[kernel]  # its list sits in the tail pool: the general path took it
        if kind != "equal":
            _assert_same(outs["equal"], out, kind)
    blocks = {kind: int(np.nonzero(o["order"] == dense_tile)[0][0]) for kind, o in outs.items()}
    assert len(set(blocks.values())) > 1, blocks  # the dense tile was moved


@pytest.mark.parametrize("views,hw,n", [(3, (256, 256), 8000), (1, (128, 96), 8000), (1, (256, 256), 131072)])
def test_calls_outside_the_deal_are_untouched(views, hw, n):
    """Three views; one view of 192 tiles (fewer tiles than compute units); one view whose binning launch has a workgroup on every
    compute unit (131 072 Gaussians: 256 rows, no room for the table's builders): image order as before - the table is neither
    built nor read, and the results do not depend on tile_total."""
    cfg = RasterConfig(views, 1, views, n, hw[0], hw[1], 4, 25, 4, False)
    call = _Call(cfg, 2 * call_tiles(views, hw) * 1024)
    ins = _gpu(_scene(13, n, hw, views))
    first = None
    for kind in ("zeros", "descending", "random"):
        call.hint_words(kind, ins)
        out = call.forward(ins)
        assert not torch.isnan(out["color"]).any(), kind
        assert (out["order"] == SENTINEL).all(), kind
        first = first or out
        _assert_same(first, out, kind)


def call_tiles(views, hw):
    return views * 4 * ((hw[0] + 15) // 16) * ((hw[1] + 15) // 16)


def test_the_backward_still_matches_under_two_hints():
    """A forward that announces its backward, then the backward, in GSR_FLAG_DETERMINISTIC: equal gradients whatever the forward's
    hint was (the backward deals its own tiles by the counts that forward wrote, which do not depend on the hint)."""
    flags = _lib.FLAG_BACKWARD_FOLLOWS | _lib.FLAG_DETERMINISTIC
    cfg = RasterConfig(1, 1, 1, N, HW[0], HW[1], 4, 25, 4, False, flags)
    call = _Call(cfg, 2 * T * 1024, backward=True)
    ins = _gpu(_scene(11))
    g_color = torch.rand((1, 3) + HW, generator=torch.Generator().manual_seed(3)).to(_dev())
    grads = []
    for kind in ("ascending", "random"):
        call.hint_words(kind, ins)
        out = call.forward(ins)
        assert not np.array_equal(out["order"], np.arange(T))
        call.be.run_backward(call.plan, *ins, None, g_color)
        torch.cuda.synchronize()
        grads.append({k: call.plan[k].cpu().clone() for k in ("d_means", "d_cov6", "d_opac", "d_colors", "d_means2d")})
    for k, g in grads[0].items():
        assert torch.isfinite(g).all() and bool((g != 0).any()), k
        assert torch.equal(g, grads[1][k]), k
