"""`-m gpu`: the forward tile launch's deal by the measured time model (pf3plat_amd/csrc/gsr_common.h: build_tile_order_model).  The
binning launch builds the table from what the plan's PREVIOUS forward left per tile - walked entries (tile_total) and list length
(ranges).  The device's table must be the host statement's (gsr_tile_deal_order: integer arithmetic on both sides), a permutation
of each XCD's tiles whatever those words hold, and placement must not touch a bit of the results.

Shapes: one view of 136 x 136 (the smallest image the deal is active for: more 8 x 8 tiles than the 256 compute units) and one of
256 x 256 (1024 tiles: four full slots per compute unit), 6 000 Gaussians each.  Every comparison is exact.
Scenes of this size list a few dozen keys per tile, and an XCD of such lists keeps the shipped order (kDealMinMeanList): the exchanges
themselves run in the cases that write headline-like words - 224 ... 448 walked entries, lists of 600 ... 1700 keys, as ranges the tile launch would have written - where the builder reads.
The table's other builder, k_tile_order, runs only on a device that does not grant the binning launch its LDS: no case here reaches it."""
import ctypes

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib
from pf3plat_amd.rasterizer import RasterConfig
from tests.test_gpu_tile_deal import SENTINEL, _assert_same, _Call, _gpu, _scene

pytestmark = pytest.mark.gpu

N = 6000
SHAPES = ((136, 136), (256, 256))


def _host_table(walked, length, tiles):
    """The table gsr_tile_deal_order defines for `tiles` tiles: XCD x owns a contiguous run, its k-th workgroup is block 8 k + x."""
    lib, P = _lib.load(), ctypes.POINTER(ctypes.c_uint32)
    out = np.zeros(tiles, dtype=np.int64)
    q, r = tiles >> 3, tiles & 7
    for x in range(8):
        base, cnt = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q), q + (1 if x < r else 0)
        w = np.ascontiguousarray(walked[base: base + cnt], dtype=np.uint32)
        n = np.ascontiguousarray(length[base: base + cnt], dtype=np.uint32)
        o = np.zeros(cnt, dtype=np.uint32)
        assert lib.gsr_tile_deal_order(w.ctypes.data_as(P), n.ctypes.data_as(P), cnt, o.ctypes.data_as(P)) == 0
        out[x::8][:cnt] = base + o.astype(np.int64)
    return out


def _words_left(call, stride, tiles):
    """What the next call's builder will read: (tile_total, list lengths) as unsigned words."""
    torch.cuda.synchronize()
    tt = call.words("tile_total").cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    rg = call.plan["bin"][call.lay["ranges"]: call.lay["ranges"] + 8 * call.VT].view(torch.int32).reshape(call.VT, 2).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    # a list length counts where the words are a range the tile launch writes for that tile (gsr.h: gsr_tile_deal_order), else 0
    n, t = (rg[:, 1] - rg[:, 0]) & 0xFFFFFFFF, np.arange(call.VT)
    own = (rg[:, 0] == (t * stride) & 0xFFFFFFFF) & (n <= stride)
    tail = (rg[:, 0] >= tiles * stride) & (n > stride)
    return tt, np.where(own | tail, n, 0)


def _check_table(out, walked, length, what):
    order = out["order"]
    tiles = int((order != SENTINEL).sum())  # the builder writes one word per tile of the grid
    assert 256 < tiles <= len(order) and (order[:tiles] != SENTINEL).all(), (what, tiles)
    assert np.array_equal(np.sort(order[:tiles]), np.arange(tiles)), what  # a permutation
    q, r = tiles >> 3, tiles & 7
    for x in range(8):
        base, cnt = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q), q + (1 if x < r else 0)
        mine = order[:tiles][x::8]
        assert len(mine) == cnt and mine.min() >= base and mine.max() < base + cnt, (what, x)  # every tile on its own XCD
    assert np.array_equal(order[:tiles], _host_table(walked, length, tiles)), what
    return tiles


@pytest.mark.parametrize("hw", SHAPES)
def test_the_table_is_the_host_statements_and_the_bits_do_not_move(hw):
    cfg = RasterConfig(1, 1, 1, N, hw[0], hw[1], 4, 25, 4, False)
    tiles_padded = 4 * ((hw[0] + 15) // 16) * ((hw[1] + 15) // 16)
    call = _Call(cfg, 2 * tiles_padded * 700)  # (slot 700: k_tile_fwd_prefix)
    ins = _gpu(_scene(21, N, hw))
    first = call.forward(ins)
    assert not torch.isnan(first["color"]).any()
    stride = int(first["range_start"][1])  # (tile 1's list sits in its own slot: a few dozen keys)
    tiles = int((first["order"] != SENTINEL).sum())
    assert stride >= 700 and int(first["range_start"][2]) == 2 * stride
    # the second forward: dealt by what the first left
    walked, length = _words_left(call, stride, tiles)
    second = call.forward(ins)
    assert tiles == _check_table(second, walked, length, "second forward")
    assert int(walked[:tiles].max()) > int(walked[:tiles].min())  # a real load profile
    assert not np.array_equal(second["order"], first["order"])  # ... which moved tiles
    _assert_same(first, second, "second forward")
    # after a call that overflowed its pair workspace: every footprint 2500 x the area
    vb, means, cov6, opac, colors = ins
    call.be.run_forward(call.plan, vb, means, cov6 * 2500.0, opac, colors)
    assert call.be.read_status(call.plan)["overflow"] == 1
    walked, length = _words_left(call, stride, tiles)
    third = call.forward(ins)
    _check_table(third, walked, length, "after an overflowed call")
    _assert_same(first, third, "after an overflowed call")
    # headline-like words where the builder reads: the exchanges run on the device (the shipped order alone would not match)
    g = torch.Generator().manual_seed(9)
    call.words("tile_total").copy_(32 * torch.randint(7, 15, (call.VT,), generator=g, dtype=torch.int32))  # (whole batches, as a blend leaves)
    rg = torch.zeros(call.VT, 2, dtype=torch.int32)
    rg[:, 0] = torch.arange(call.VT, dtype=torch.int32) * stride  # (every list in its tile's own slot, or longer than it and in the tail pool)
    rg[:, 1] = rg[:, 0] + torch.randint(600, 701, (call.VT,), generator=g, dtype=torch.int32)
    long_ = torch.arange(call.VT) % 5 == 0
    rg[long_, 0] = tiles * stride + 7
    rg[long_, 1] = rg[long_, 0] + torch.randint(701, 1701, (int(long_.sum()),), generator=g, dtype=torch.int32)
    call.plan["bin"][call.lay["ranges"]: call.lay["ranges"] + 8 * call.VT].view(torch.int32).copy_(rg.reshape(-1))
    walked, length = _words_left(call, stride, tiles)
    exchanged = call.forward(ins)
    _check_table(exchanged, walked, length, "headline-like words")
    call.words("tile_total").copy_(torch.from_numpy(walked.astype(np.int32)))  # the same counts over the scene's own short lists
    torch.cuda.synchronize()
    plain = call.forward(ins)
    assert not np.array_equal(exchanged["order"], plain["order"])  # the exchanges moved tiles
    _assert_same(first, exchanged, "headline-like words")
    # the words the builder reads filled with 0xff bytes
    call.words("tile_total").fill_(-1)
    call.plan["bin"][call.lay["ranges"]: call.lay["ranges"] + 8 * call.VT].fill_(0xFF)
    walked, length = _words_left(call, stride, tiles)
    assert (walked == 0xFFFFFFFF).all()
    fourth = call.forward(ins)
    _check_table(fourth, walked, length, "0xff words")
    _assert_same(first, fourth, "0xff words")
