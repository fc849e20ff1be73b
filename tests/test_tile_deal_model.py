"""The forward tile launch's deal by the measured time model (pf3plat_amd/csrc/gsr_common.h: deal_term, tile_deal_order_host), through
the library's host entry gsr_tile_deal_order - integer arithmetic, the statement the device's builder is tested against
(tests/test_gpu_tile_deal_model.py).  No GPU.

  * whatever the words hold, the answer is a permutation of the XCD's tiles;
  * on recorded (walked entries, list length) pairs - the seed-2 scene at 200 000 Gaussians (lists of 418 - 1117 keys), from tests/tile_walk_sim.py (tile_lists,
    walk), committed as tests/golden/tile_deal_pairs_seed2_n200000.npz - the modelled slowest compute unit of the answer is never
    above the shipped order's (heaviest first, every other round of 32 mirrored: the order the search starts from);
  * an XCD whose tiles list fewer than 512 keys on average - outside the range the model was measured on - or whose words are not what
    a forward leaves keeps the shipped order."""
import ctypes
import os

import numpy as np
import pytest

from pf3plat_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_deal_pairs_seed2_n200000.npz")
COUNTS = (33, 64, 65, 127, 128, 256, 20)  # tiles per XCD; 20: fewer than its 32 compute units
CLAMP = 0x3FFF
WN, WL = (294, 294, 249, 1432), (35, 23, 17, 26)  # deal_term's weights by slot, 2^-16 us per walked entry / per list entry


def deal(walked, length):
    walked, length = (np.ascontiguousarray(a, dtype=np.uint32) for a in (walked, length))
    out = np.full(len(walked), 0xFFFFFFFF, dtype=np.uint32)
    P = ctypes.POINTER(ctypes.c_uint32)
    rc = _lib.load().gsr_tile_deal_order(walked.ctypes.data_as(P), length.ctypes.data_as(P), len(walked), out.ctypes.data_as(P))
    assert rc == 0, rc
    return out.astype(np.int64)


def shipped_order(walked):
    """Heaviest first by (min(count, 0xfffffe) + 1) << 8 | (255 - index); workgroup k takes position (k >> 5) << 5 | in, mirrored in odd rounds."""
    cnt = len(walked)
    keys = ((np.minimum(walked.astype(np.int64), 0xFFFFFE) + 1) << 8) | (255 - np.arange(cnt))
    by_load = np.argsort(-keys, kind="stable")
    out = np.zeros(cnt, dtype=np.int64)
    for k in range(cnt):
        rnd, j = k >> 5, k & 31
        ln = min(32, cnt - (rnd << 5))
        out[k] = by_load[(rnd << 5) + (ln - 1 - j if rnd & 1 else j)]
    return out


def modelled_units(order, walked, length):
    """Cost of each of the XCD's 32 compute units under `order` (slot k >> 5 on unit k & 31), in 2^-16 us."""
    cost = np.zeros(32, dtype=np.int64)
    for k, t in enumerate(order):
        s = k >> 5
        cost[k & 31] += WN[s] * min(int(walked[t]), CLAMP) + WL[s] * min(int(length[t]), CLAMP)
    return cost


def _patterns(cnt):
    rng = np.random.default_rng(cnt)
    yield "random", rng.integers(0, 600, cnt), rng.integers(0, 2000, cnt)
    yield "headline-like", 32 * rng.integers(7, 15, cnt), rng.integers(600, 1700, cnt)
    yield "zeros", np.zeros(cnt, np.int64), np.zeros(cnt, np.int64)
    yield "equal", np.full(cnt, 320), np.full(cnt, 1200)
    yield "garbage", np.full(cnt, 0xFFFFFFFF), np.full(cnt, 0xFFFFFFFF)
    yield "random words", rng.integers(0, 1 << 32, cnt), rng.integers(0, 1 << 32, cnt)
    yield "one heavy", np.where(np.arange(cnt) == cnt // 2, 448, 224), rng.integers(600, 1700, cnt)


@pytest.mark.parametrize("cnt", COUNTS)
def test_a_permutation_whatever_the_words_hold(cnt):
    for name, walked, length in _patterns(cnt):
        order = deal(walked, length)
        assert np.array_equal(np.sort(order), np.arange(cnt)), (cnt, name)


def test_more_than_128_tiles_keep_the_shipped_order():
    """The model deals four slots x 32 units; a longer XCD (no call of the forward's deal has one) keeps heaviest first, mirrored."""
    rng = np.random.default_rng(1)
    walked, length = rng.integers(0, 600, 256), rng.integers(0, 2000, 256)
    assert np.array_equal(deal(walked, length), shipped_order(walked))


@pytest.mark.parametrize("cnt", (37, 128))
def test_short_lists_keep_the_shipped_order(cnt):
    """Mean list length below 512 (kDealMinMeanList): no exchange, whatever the counts; at 512 and above the search runs."""
    rng = np.random.default_rng(cnt + 1)
    walked = 32 * rng.integers(7, 15, cnt)
    short = np.full(cnt, 511)
    short[0] = 510 + cnt  # the sum one short of 512 x cnt
    assert np.array_equal(deal(walked, short), shipped_order(walked))
    assert np.array_equal(deal(walked, np.zeros(cnt, np.int64)), shipped_order(walked))  # a fresh workspace
    long_ = rng.integers(600, 1700, cnt)
    order = deal(walked, long_)
    assert not np.array_equal(order, shipped_order(walked))
    assert modelled_units(order, walked, long_).max() < modelled_units(shipped_order(walked), walked, long_).max()
    # words a forward does not leave: one tile that walked a part batch, more than its list, or nothing of a list with entries
    for bad in (walked[3] + 5, long_[3] + 32, 0):
        odd = walked.copy()
        odd[3] = bad
        assert np.array_equal(deal(odd, long_), shipped_order(odd)), bad
    whole = walked.copy()
    whole[3] = long_[3]  # the whole list: plausible
    assert np.array_equal(np.sort(deal(whole, long_)), np.arange(cnt))


def test_bad_arguments_are_refused():
    P = ctypes.POINTER(ctypes.c_uint32)
    a = np.zeros(300, np.uint32)
    lib = _lib.load()
    for cnt in (0, -1, 257):
        assert lib.gsr_tile_deal_order(a.ctypes.data_as(P), a.ctypes.data_as(P), cnt, a.ctypes.data_as(P)) != 0


@pytest.mark.parametrize("cnt", (128, 100, 64, 37))
def test_the_modelled_slowest_unit_is_never_above_the_shipped_orders(cnt):
    z = np.load(GOLDEN)
    walked_all, length_all = z["walked"].astype(np.int64), z["list_length"].astype(np.int64)
    assert len(walked_all) == 1024 and walked_all.max() > walked_all.min()
    improved = 0
    for x in range(1024 // cnt):
        walked, length = walked_all[x * cnt: (x + 1) * cnt], length_all[x * cnt: (x + 1) * cnt]
        order = deal(walked, length)
        assert np.array_equal(np.sort(order), np.arange(cnt))
        new, old = modelled_units(order, walked, length).max(), modelled_units(shipped_order(walked), walked, length).max()
        assert new <= old, (cnt, x, new, old)
        improved += new < old
    assert improved > 0  # the search did something on a real load profile
