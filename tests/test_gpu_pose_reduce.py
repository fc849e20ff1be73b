"""The camera-gradient reductions (`k_pose_reduce<35|37>`, `k_pose_reduce_z`, csrc/gsr_backward.h) at training-scale Gaussian counts.

`k_preprocess_bwd` leaves partial rows in `pose_partials`; the reduce kernels add them up in two levels (one for the depth-only
gradient below 16 385 rows).  After `HipBackend.run_backward(plan, ..., d_views=...)` the rows are still in `plan["pose_partials"]`,
level 0 `[V][rows1][kCols]` and directly behind it level 1 `[V][blocks][kCols]`, so the reduction can be checked on its own, exactly:
`check_reduction` below compares both levels of a call with float64 sums of that call's own level-0 rows.

The bounds of `check_reduction`, derived (nothing here is measured).  u = 2^-24 is the unit roundoff of float32.  A sum formed by
float additions in which every input passes through at most n roundings differs from the exact sum by at most
gamma_n sum|x|, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: the (n-1) u bound of a
summation chain of n terms, for any order).  A reducing block gives thread row r0 the rows r_begin + r0, + kRows, ...: at most
ceil(per / kRows) terms added one after the other onto 0.0f, then one thread adds the kRows results onto 0.0f.  The first addition
of each chain (0 + x) is exact, so an input sees at most ceil(per / kRows) + kRows - 2 roundings.  The check allows
L = ceil(per / kRows) + kRows of them, L u sum|x|: the two spare units cover the denominator of gamma (gamma_{L-2} <= L u as long as
L (L - 2) <= 2^25, L <= 5792; the largest L here is 1 + 64 + 5 + 64 = 134) and the rounding of the float64 reference sum (at most 2^-53 x
16 386 of sum|x|).  The second level adds chains of the same form over the first level's rows, so an input of level 0 reaches the
record through at most (L1 - 2) + (L2 - 2) roundings and the record may differ from the float64 sum of ALL level-0 rows by
(L1 + L2) u sum|x|.  kRows = 256 // kCols (7 for 35 columns, 6 for 37); the depth-only kernel adds 64 rows of 4 floats per step, 64
takes the place of kRows.  A block past the last row adds nothing: exact zeros.

(b) of the GPU cases compares a scene with its compact twin (its live Gaussians alone).  Both calls reduce the same per-Gaussian
contributions: the large call's rows hold one live Gaussian per 16-lane group (its row sums are exact, x + 0 + ...), the twin's hold 16,
added by four DPP steps (4 u sum|contribution| = 2^-22 sum|rows of the large call|); the depth-only rows add two more steps on both
sides, which the spare units of the two section-1 bounds cover.  The cotangent rows the contributions are computed from are themselves
sums of float atomics over pixels, in an order that changes from run to run; the twin is therefore run twice and the bound is widened
by 4 x sum|row difference between the twin's two runs| - never against the large call.  That difference is a sample, and a sound
one only where thousands of rows enter it.  The five live Gaussians of `small` do not give one: with make_scene's cameras (rotation I,
no translation along z) the view-matrix entries 8 and 9 have no gradient analytically - pose[9] = dty mz + dM[5] J11 = -fy dM[5] / mz +
fy dM[5] / mz - so what the kernel leaves there is the rounding of that cancellation, which a last-bit change of a cotangent row
turns over entirely; on the MI355X the large call differed from the twin by 1.7 x sum|rows| in column 9 (2.7e5 bounds) while the twin's
own two runs happened to agree there.  `small` and `small_z` therefore do (b) on a pair of calls that carry GSR_FLAG_DETERMINISTIC,
whose cotangent rows are fixed-point sums - the same bits in both calls and in every run (asserted), the same reduce kernels - so
the bound holds there with no widening at all; (a) and (c) stay on the call without the flag.  docs/PARITY.md 9.1 has the measured
figures.

The scenes: in every run of 16 consecutive indices one Gaussian at a seeded position is live and the other 15 are inert - behind
every camera or far outside every frustum, radius 0 in every view for the oracle.  Every level-0 row then has a contributor while
oracle and blend cost stay those of N / 16 Gaussians.  The live ones are `synthetic.make_scene`'s population for the 64 x 64 image
(near 1.25), with two departures that the conditions on a case force.  As the generator draws them, 15 % of a population lie outside
one of the two render cameras' images (they are un-projected from source cameras half a unit to either side), and of 8 195 of them on
4 096 pixels the nearer ones hide the rest: the float32 oracle touches 59 % of the rows (seed 1), a property of the population that no seed brings to 90 %.
Hence (i) twice as many are drawn and those whose centre projects two pixels inside every view's image are kept (`_on_screen`,
evenly over the draw, in order), and (ii) their opacities are multiplied by 0.1, which keeps the transmittance of a pixel above the
1e-4 at which a blend stops.  With that the oracle alone touches over 99.8 % of the 16-lane rows of every full-gradient case and 98 %
of z_two's 64-lane rows: `test_scene_construction_by_the_oracle_alone` holds every scene to the conditions on the CPU, the GPU cases
assert them again on the kernels' own rows."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, rasterizer, synthetic
from pf3plat_amd.rasterizer import RasterConfig
from tests import gpu_util, parity_checks
from tests.camera_rig import Case

U = 2.0 ** -24
POSE_BLOCKS = 256    # kPoseBlocks
Z_BLOCKS = 64        # level-1 blocks of k_pose_reduce_z when it takes two levels
Z_ONE_LEVEL = 16384  # ... which it does above this many rows
Z_SLOTS = (2, 6, 10, 14)
HW = (64, 64)
NEAR = 1.25
OPACITY = 0.1  # factor on make_scene's opacities (module docstring: the live Gaussians)
DEPTH, DET, FOV = 1 << 4, _lib.FLAG_DETERMINISTIC, _lib.FLAG_FOV_GRADIENT
MIN_SHARE = 0.9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cdiv(a, b):
    return -(-a // b)


def geometry(n, k_cols):
    """-> (rows1, level-1 blocks or None, per) of a call with n Gaussians and rows of k_cols floats (4: the depth-only gradient)."""
    units = _cdiv(n, 64)
    if k_cols == 4:
        blocks = None if units <= Z_ONE_LEVEL else Z_BLOCKS
        return units, blocks, None if blocks is None else _cdiv(units, blocks)
    return 4 * units, POSE_BLOCKS, _cdiv(4 * units, POSE_BLOCKS)


def chain(rows, k_rows):
    """Longest chain of float additions of one reducing block over `rows` rows (module docstring)."""
    return _cdiv(rows, k_rows) + k_rows


# ---- section 1: the exact check ---------------------------------------------------------------------------------------------------
def check_reduction(level0, level1, d_views, k_cols, blocks):
    """level0 (V, rows1, k_cols) float32 rows, level1 (V, blocks, k_cols) or None (one level), d_views (V, 48), all of ONE call.
    Asserts per view and column what the module docstring derives; -> dict(share1, share2: worst |error| / bound of each level,
    bound2: the (V, k_cols) level-2 bounds, abs_sum: (V, k_cols) sum|x|).  Pure numpy, float64 sums."""
    level0 = np.asarray(level0)
    d_views = np.asarray(d_views)
    assert level0.dtype == np.float32 and d_views.dtype == np.float32 and level0.ndim == 3 and level0.shape[2] == k_cols
    v, rows1, _ = level0.shape
    assert d_views.shape == (v, 48)
    k_rows = 64 if k_cols == 4 else 256 // k_cols
    x = level0.astype(np.float64)
    ax = np.abs(x)
    assert np.isfinite(x).all(), "non-finite level-0 rows (or rows the first stage never wrote)"
    out = dict(share1=0.0)
    l1 = 0
    if level1 is not None:
        level1 = np.asarray(level1)
        assert level1.dtype == np.float32 and level1.shape == (v, blocks, k_cols)
        per = _cdiv(rows1, blocks)
        l1 = chain(per, k_rows)
        pad = ((0, 0), (0, blocks * per - rows1), (0, 0))  # (per = ceil: blocks * per >= rows1; the padding rows are exact zeros)
        s1 = np.pad(x, pad).reshape(v, blocks, per, k_cols).sum(2)
        a1 = np.pad(ax, pad).reshape(v, blocks, per, k_cols).sum(2)
        e1, b1 = np.abs(level1.astype(np.float64) - s1), l1 * U * a1
        bad = np.argwhere(~(e1 <= b1))
        assert bad.size == 0, ("level 1", len(bad), "first (view, block, column)", bad[0].tolist(), "error", e1[tuple(bad[0])], "bound", b1[tuple(bad[0])])
        first_empty = _cdiv(rows1, per)
        assert not _bits(level1[:, first_empty:]).any(), "a level-1 block past the last row is not zero"
        out["share1"] = float((e1[b1 > 0] / b1[b1 > 0]).max(initial=0.0))
    l2 = chain(rows1 if level1 is None else blocks, k_rows)
    cols = list(Z_SLOTS) if k_cols == 4 else list(range(k_cols))
    total, atot = x.sum(1), ax.sum(1)
    e2, b2 = np.abs(d_views[:, cols].astype(np.float64) - total), (l1 + l2) * U * atot
    bad = np.argwhere(~(e2 <= b2))
    assert bad.size == 0, ("level 2", len(bad), "first (view, column)", bad[0].tolist(), "error", e2[tuple(bad[0])], "bound", b2[tuple(bad[0])])
    rest = np.ones(48, bool)
    rest[cols] = False
    assert not _bits(d_views[:, rest]).any(), "a record entry outside the gradient's columns is not zero"
    out.update(share2=float((e2[b2 > 0] / b2[b2 > 0]).max(initial=0.0)), bound2=b2, abs_sum=atot)
    return out


# ---- float32 emulation of the kernels' summation order (the CPU tests of the check) ------------------------------------------------------
def _emulate_level(x, blocks, k_rows, floor_per=False):
    """One launch of k_pose_reduce / k_pose_reduce_z over x (V, rows, k) float32 with `blocks` blocks per view -> (V, blocks, k): thread
    row r0 of block b adds rows r_begin + r0, + k_rows, ... one after the other (the four loads of the unrolled loop are added in that
    order too), then the k_rows results are added in order.  floor_per: the mutant that takes per = rows // blocks."""
    v, rows, k = x.shape
    per = max(1, rows // blocks) if floor_per else _cdiv(rows, blocks)
    out = np.zeros((v, blocks, k), np.float32)
    for b in range(blocks):
        r_begin, r_end = b * per, min(rows, b * per + per)
        s = np.zeros((v, k), np.float32)
        for r0 in range(k_rows):
            acc = np.zeros((v, k), np.float32)
            for r in range(r_begin + r0, r_end, k_rows):
                acc = acc + x[:, r]
            s = s + acc
        out[:, b] = s
    return out


def emulate(level0, k_cols, blocks, floor_per=False, stride2=None):
    """-> (level1 or None, d_views (V, 48)) as the kernels form them from level0 (V, rows1, k_cols), in float32.  stride2: the mutant
    whose second level reads the level-1 buffer as rows of `stride2` floats (the other instance of the template)."""
    level0 = np.asarray(level0, np.float32)
    v = level0.shape[0]
    k_rows = 64 if k_cols == 4 else 256 // k_cols
    level1 = None if blocks is None else _emulate_level(level0, blocks, k_rows, floor_per)
    src = level0 if level1 is None else level1
    if stride2 is not None:
        src = src.reshape(-1)[:v * blocks * stride2].reshape(v, blocks, stride2)
        k_rows = 256 // stride2
    sums = _emulate_level(src, 1, k_rows)[:, 0]
    d_views = np.zeros((v, 48), np.float32)
    d_views[:, list(Z_SLOTS) if k_cols == 4 else list(range(sums.shape[1]))] = sums
    return level1, d_views


def seeded_rows(seed, v, rows, k_cols):
    """Rows of either sign whose magnitudes spread log-uniformly over three decades."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((v, rows, k_cols)) * 10.0 ** rng.uniform(-3, 0, (v, rows, 1))).astype(np.float32)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Spec:
    n: int
    k_cols: int
    seed: int
    views: int = 2
    sets: int = 1
    flags: int = 0
    rows1: int = 0   # what the case is for (asserted against `geometry`)
    per: int = 0
    twin_det: bool = False  # (b) on a pair of calls that carry GSR_FLAG_DETERMINISTIC


CASES = {
    "below": Spec(86016, 35, seed=1, rows1=5376, per=21),
    "edge": Spec(90112, 35, seed=1, sets=2, rows1=5632, per=22),
    "model": Spec(131109, 35, seed=1, rows1=8196, per=33),
    "model_det": Spec(131109, 35, seed=1, flags=DET, rows1=8196, per=33),
    "two_trips": Spec(229441, 35, seed=1, rows1=14344, per=57),
    "fov": Spec(131109, 37, seed=1, flags=FOV, rows1=8196, per=33),
    "z_one": Spec(131109, 4, seed=1, rows1=2049),
    "z_two": Spec(1048641, 4, seed=1, rows1=16386, per=257),
    "small": Spec(65, 35, seed=1, rows1=8, per=1, twin_det=True),
    "small_z": Spec(65, 4, seed=1, rows1=2, twin_det=True),
}


def live_positions(seed, n):
    """One index per run of 16 (the last run may be short): seeded, a pure function of (seed, n)."""
    runs = _cdiv(n, 16)
    start = 16 * np.arange(runs)
    length = np.minimum(16, n - start)
    return start + np.minimum((np.random.default_rng(seed).random(runs) * length).astype(np.int64), length - 1)


def _on_screen(records, means, margin=2.0):
    """Indices of the Gaussians whose centre projects at least `margin` pixels inside the image of every one of the (V, 48) camera
    records (float64 from the records' projection matrix and scale)."""
    ok = np.ones(len(means), bool)
    for f in records.astype(np.float64):
        m = means.astype(np.float64) * f[40]
        w = f[19] * m[:, 0] + f[23] * m[:, 1] + f[27] * m[:, 2] + f[31]
        for axis, size in ((0, HW[1]), (1, HW[0])):
            ndc = (f[16 + axis] * m[:, 0] + f[20 + axis] * m[:, 1] + f[24 + axis] * m[:, 2] + f[28 + axis]) / w
            pix = ((ndc + 1.0) * size - 1.0) * 0.5
            ok &= (w > 0) & (pix >= margin) & (pix <= size - 1 - margin)
    return np.flatnonzero(ok)


@functools.lru_cache(maxsize=2)
def scene(name, compact=False):
    """-> (Case, live index array).  compact: the twin - the live Gaussians alone, in the same order, under the same cameras and
    cotangents.  CPU tensors; built once per case and left unchanged."""
    sp = CASES[name]
    n, live = sp.n, live_positions(sp.seed, sp.n)
    scs = [synthetic.make_scene(sp.seed + 1000 * s, 2 * len(live), HW, d_sh=25, num_views=sp.views, near=NEAR) for s in range(sp.sets)]
    vb = torch.cat([gpu_util.scene_viewbuf(sc) for sc in scs])
    parts = []
    for s, sc in enumerate(scs):
        ok = _on_screen(vb[s * sp.views:(s + 1) * sp.views].numpy(), sc.gaussians.means[0].numpy())
        assert len(ok) >= len(live)
        keep = torch.from_numpy(ok[np.linspace(0, len(ok) - 1, len(live)).astype(np.int64)])  # evenly from both source cameras, in order
        parts.append([t[:, keep] for t in gpu_util.scene_tensors(sc)])
    means, cov, opac, colors = (torch.cat([p[k] for p in parts]).contiguous() for k in range(4))
    opac = opac * OPACITY
    rng = np.random.default_rng(sp.seed)
    v = sp.sets * sp.views
    gc = torch.tensor(rng.uniform(0, 1, (v, 3, *HW)).astype(np.float32))
    ge = torch.tensor(rng.uniform(0, 1, (v, *HW)).astype(np.float32))
    if not compact:
        # inert Gaussians: even indices behind every camera (the cameras look along +z from around the origin), odd ones far to
        # the side of every frustum (|x| / z >= 6 against tan-fov 0.58); small, so that no footprint reaches the image
        g = torch.Generator().manual_seed(sp.seed + 77)
        r = torch.rand((sp.sets, n, 3), generator=g)
        behind = torch.stack((6 * r[..., 0] - 3, 6 * r[..., 1] - 3, -1 - 19 * r[..., 2]), -1)
        side = torch.stack((torch.where(r[..., 0] < 0.5, -1.0, 1.0) * (60 + 30 * r[..., 1]), 6 * r[..., 1] - 3, 2 + 8 * r[..., 2]), -1)
        full_means = torch.where((torch.arange(n) % 2 == 0)[None, :, None], behind, side)
        full_cov = torch.tensor([1e-4, 0, 0, 1e-4, 0, 1e-4]).repeat(sp.sets, n, 1)
        full_opac = torch.full((sp.sets, n), 0.5)
        full_colors = torch.full((sp.sets, n, 25, 3), 0.1)
        idx = torch.from_numpy(live)
        full_means[:, idx], full_cov[:, idx], full_opac[:, idx], full_colors[:, idx] = means, cov, opac, colors
        means, cov, opac, colors = full_means, full_cov, full_opac, full_colors
    cfg = RasterConfig(v, sp.sets, sp.views, means.shape[1], *HW, 4, 25, 4, True, DEPTH | sp.flags)
    return Case(cfg, vb, means.contiguous(), cov.contiguous(), opac.contiguous(), colors.contiguous(), None, gc, ge), live


def populated_rows(n, k_cols):
    """Level-0 rows that hold a Gaussian at all: 16 lanes per row (64 for the depth-only row).  The rows of a partial last workgroup
    behind them hold none and must be zero."""
    return _cdiv(n, 64 if k_cols == 4 else 16)


def oracle_row_share(o, live, n, k_cols):
    """From an oracle result WITH gradients: per view, the share of populated level-0 rows in which a live Gaussian received a
    non-zero screen-space gradient (what `k_preprocess_bwd` takes as "the blend touched it")."""
    m2d = o["grads"]["means2d"]
    lanes = 64 if k_cols == 4 else 16
    shares = []
    for v in range(m2d.shape[0]):
        touched = np.zeros(populated_rows(n, k_cols), bool)
        hit = live[(m2d[v][live] != 0).any(-1)]
        touched[hit // lanes] = True
        shares.append(float(touched.mean()))
    return shares


def check_construction(radii, live, n):
    """Oracle radii (V, n) of the large scene: a live Gaussian with radius > 0 in every run of 16 and every view, radius 0 for
    every inert one."""
    radii = np.asarray(radii)
    inert = np.ones(n, bool)
    inert[live] = False
    assert len(live) == _cdiv(n, 16) and (live // 16 == np.arange(len(live))).all()
    assert not radii[:, inert].any(), ("inert Gaussians with a footprint", int((radii[:, inert] != 0).sum()))
    assert (radii[:, live] > 0).all(), ("live Gaussians without a footprint", int((radii[:, live] <= 0).sum()))


# ---- CPU tests: the check itself, and the host arithmetic ------------------------------------------------------------------------------
EMULATED = [(name, sp.rows1, sp.k_cols) for name, sp in CASES.items() if name != "model_det"]


@pytest.mark.parametrize("name,rows1,k_cols", EMULATED)
def test_check_accepts_the_faithful_emulation(name, rows1, k_cols):
    sp = CASES[name]
    r1, blocks, per = geometry(sp.n, k_cols)
    assert (r1, per or 0) == (rows1, sp.per)
    x = seeded_rows(10 + rows1 + k_cols, 2, rows1, k_cols)
    level1, d_views = emulate(x, k_cols, blocks)
    m = check_reduction(x, level1, d_views, k_cols, blocks)
    assert 0 < m["share2"] < 1 and m["share1"] < 1
    assert m["share1"] > 0 or blocks is None or per == 1  # (one row per block: the first level copies)


@pytest.mark.parametrize("k_cols,rows1,blocks", [(35, 8196, 256), (37, 8196, 256), (4, 16386, 64)])
def test_check_rejects_a_dropped_a_doubled_and_a_floor_partition(k_cols, rows1, blocks):
    x, per = seeded_rows(3, 2, rows1, k_cols), _cdiv(rows1, blocks)
    check_reduction(x, *emulate(x, k_cols, blocks), k_cols, blocks)
    # the smallest-magnitude non-zero row of one block dropped; the smallest of another added twice
    for view, block, factor in ((1, 5, 0.0), (0, blocks // 2, 2.0)):
        rows = slice(block * per, block * per + per)
        mag = np.abs(x[view, rows]).max(-1)
        r = block * per + int(np.argmin(np.where(mag > 0, mag, np.inf)))
        y = x.copy()
        y[view, r] *= np.float32(factor)
        with pytest.raises(AssertionError, match="level 1"):
            check_reduction(x, *emulate(y, k_cols, blocks), k_cols, blocks)
    assert rows1 % blocks  # per = floor loses the last rows1 - blocks * floor rows
    with pytest.raises(AssertionError, match="level 1"):
        check_reduction(x, *emulate(x, k_cols, blocks, floor_per=True), k_cols, blocks)
    level1, _ = emulate(x, k_cols, blocks)
    with pytest.raises(AssertionError, match="level 2"):
        check_reduction(x, level1, emulate(x, k_cols, blocks, floor_per=True)[1], k_cols, blocks)


def test_check_rejects_a_second_level_at_the_other_stride():
    x = seeded_rows(4, 2, 8196, 37)
    level1, d_views = emulate(x, 37, 256, stride2=35)
    with pytest.raises(AssertionError, match="level 2"):
        check_reduction(x, level1, d_views, 37, 256)
    # the record entries behind the columns, and a row the first stage never wrote
    level1, d_views = emulate(x, 37, 256)
    d_views[1, 40] = 1e-30
    with pytest.raises(AssertionError, match="outside"):
        check_reduction(x, level1, d_views, 37, 256)
    x[0, 8195, 3] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_reduction(x, *emulate(x, 37, 256), 37, 256)


def test_depth_only_record_layout_is_checked():
    x = seeded_rows(5, 2, 2049, 4)
    _, d_views = emulate(x, 4, None)
    check_reduction(x, None, d_views, 4, None)
    moved = np.zeros_like(d_views)
    moved[:, :4] = d_views[:, list(Z_SLOTS)]
    with pytest.raises(AssertionError):
        check_reduction(x, None, moved, 4, None)


def test_pose_partials_bytes_cover_both_levels():
    lib = _lib.load()
    for name, sp in CASES.items():
        v = sp.views * sp.sets
        d = _lib.GsrDims(_lib.GSR_ABI_VERSION, v, sp.sets, sp.views, sp.n, *HW, 4, 25, 4, 1, DEPTH | sp.flags, 1 << 16)
        have = lib.gsr_pose_partials_bytes(ctypes.byref(d))
        for k_cols in {sp.k_cols, 4}:  # (a depth-only call is sized by the same function, from the same dims)
            rows1, blocks, _ = geometry(sp.n, k_cols)
            assert have >= v * (rows1 + (blocks or 0)) * k_cols * 4, (name, k_cols, have)


def test_live_positions_are_one_per_run_of_16():
    for n in (65, 131109, 1048641):
        live = live_positions(1, n)
        assert len(live) == _cdiv(n, 16) and (live // 16 == np.arange(len(live))).all() and live.max() < n
        assert len(set((live % 16).tolist())) > 1 or n < 32


@pytest.mark.parametrize("name,widths", [("below", (35,)), ("edge", (35,)), ("model", (35, 4)), ("two_trips", (35,)), ("z_two", (4,)), ("small", (35, 4))])
def test_scene_construction_by_the_oracle_alone(name, widths):
    """The conditions on a case that the reference alone must meet: radii (live > 0, inert == 0, every view), at least 90 % of the
    populated level-0 rows touched in every view - for every row width the scene is used at (fov, z_one and model_det take model's
    scene, small_z takes small's) - and a twin that renders the same image."""
    c, live = scene(name)
    t, _ = scene(name, compact=True)
    n = CASES[name].n
    assert c.cfg.num_gaussians == n and t.cfg.num_gaussians == len(live) and torch.equal(c.means[:, torch.from_numpy(live)], t.means)
    o = gpu_util.run_oracle(*c.args(), c.gc, c.ge, np.float32, True, True)
    check_construction(o["radii"], live, n)
    for k_cols in widths:
        assert min(oracle_row_share(o, live, n, k_cols)) >= MIN_SHARE, k_cols
    ot = gpu_util.run_oracle(*t.args())
    assert np.array_equal(o["color"], ot["color"]) and np.array_equal(o["extra"], ot["extra"])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _hip_call(c, depth_only, runs=1, full=False):
    """Forward + `runs` backwards of the case through the plan API -> (list of dict(level0, level1, d_views), kCols, level-1 blocks).
    The partial buffer and the record start as NaN bit patterns: whatever the kernels do not write fails the check.  full: the last
    entry also carries `res`, the image, the decoded workspaces and the other gradients in parity_checks' form."""
    dev = torch.device("cuda:0")
    be = rasterizer.HipBackend()
    cfg = c.cfg
    v, n = cfg.num_views, cfg.num_gaussians
    k_cols = 4 if depth_only else (37 if cfg.flags & FOV else 35)
    rows1, blocks, _ = geometry(n, k_cols)
    vb, means, cov, opac, colors, gc, ge = (t.to(dev).contiguous() for t in (c.vb, c.means, c.cov, c.opac, c.colors, c.gc, c.ge))
    capacity = 1 << 20
    for _ in range(2):
        plan = be.make_plan(cfg, dev, capacity, backward=True)
        be.run_forward(plan, vb, means, cov, opac, colors)
        st = be.read_status(plan)
        if not st["overflow"]:
            break
        capacity = be.capacity_for(cfg, st)
    assert not st["overflow"], st
    need = int(be.lib.gsr_pose_partials_bytes(ctypes.byref(be._sizing_dims(plan["dims"]))))
    assert need >= v * (rows1 + (blocks or 0)) * k_cols * 4
    plan["pose_partials"] = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    d_views = torch.empty((v, 48), dtype=torch.float32, device=dev)
    out = []
    for _ in range(runs):
        plan["pose_partials"].fill_(0xFF)
        d_views.fill_(float("nan"))
        be.run_backward(plan, vb, means, cov, opac, colors, None, gc, ge, True, d_views=d_views, depth_term_only=depth_only)
        torch.cuda.synchronize()
        assert plan["pose_partials"].numel() == need
        buf = plan["pose_partials"].view(torch.float32)
        n0 = v * rows1 * k_cols
        r = dict(level0=buf[:n0].reshape(v, rows1, k_cols).cpu().numpy(), level1=None, d_views=d_views.cpu().numpy())
        if blocks:
            r["level1"] = buf[n0:n0 + v * blocks * k_cols].reshape(v, blocks, k_cols).cpu().numpy()
        out.append(r)
    if not full:
        return out, k_cols, blocks
    grads = dict(means=plan["d_means"], cov6=plan["d_cov6"], opac=plan["d_opac"], colors=plan["d_colors"], extra=None, means2d=plan["d_means2d"])
    out[-1]["res"] = dict(color=plan["color"].cpu().numpy(), extra=plan["extra_img"].cpu().numpy(),
                          ws=gpu_util.decode_workspaces(be, cfg, (plan["dims"], plan["geom"], plan["bin"], plan["img"])),
                          grads={k: None if t is None else t.cpu().numpy() for k, t in grads.items()})
    return out, k_cols, blocks


def _row_share(level0, n, k_cols):
    pop = populated_rows(n, k_cols)
    assert not _bits(level0[:, pop:]).any(), "a level-0 row without a Gaussian is not zero"
    return [float((level0[v, :pop] != 0).any(-1).mean()) for v in range(level0.shape[0])]


def _case(name, oracle, runs=1):
    """(a), (b) and - oracle=True - (c) of one case; -> (the measured figures, the large call's `runs` results)."""
    sp = CASES[name]
    depth_only = sp.k_cols == 4
    c, live = scene(name)
    t, _ = scene(name, compact=True)
    n = sp.n
    bigs, k_cols, blocks = _hip_call(c, depth_only, runs=runs, full=oracle)
    big = bigs[-1]
    assert k_cols == sp.k_cols and big["level0"].shape[1] == sp.rows1
    # (a)
    ma = check_reduction(big["level0"], big["level1"], big["d_views"], k_cols, blocks)
    share = _row_share(big["level0"], n, k_cols)
    # (b)
    if sp.twin_det:  # (module docstring: a handful of Gaussians - the rows of both calls as fixed-point sums, the same bits in both)
        c_b, t = c.with_flags(DET), t.with_flags(DET)
        (big_b,), _, _ = _hip_call(c_b, depth_only)
        mb = check_reduction(big_b["level0"], big_b["level1"], big_b["d_views"], k_cols, blocks)
    else:
        big_b, mb = big, ma
    (t1, t2), _, tblocks = _hip_call(t, depth_only, runs=2)
    mt = check_reduction(t2["level0"], t2["level1"], t2["d_views"], k_cols, tblocks)
    check_reduction(t1["level0"], t1["level1"], t1["d_views"], k_cols, tblocks)
    cols = list(Z_SLOTS) if depth_only else list(range(k_cols))
    run_to_run = np.abs(t1["level0"].astype(np.float64) - t2["level0"]).sum(1)
    assert not (sp.twin_det and run_to_run.any())
    bound = mb["bound2"] + mt["bound2"] + 2.0 ** -22 * mb["abs_sum"] + 4.0 * run_to_run
    err = np.abs(big_b["d_views"][:, cols].astype(np.float64) - t2["d_views"][:, cols])
    fig = dict(share1=ma["share1"], share2=ma["share2"], twin_share=float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)),
               twin_widened=float((4.0 * run_to_run / np.maximum(bound, 1e-300)).max()), live_rows=min(share))
    print(name, {k: f"{x:.3g}" for k, x in fig.items()})
    assert (err <= bound).all(), ("twin", np.argwhere(~(err <= bound))[0].tolist(), fig)
    assert (np.abs(t2["d_views"][:, cols]).max(1) > 0).all()
    assert min(share) >= MIN_SHARE, share
    if oracle:
        o = gpu_util.run_oracle(*c.args(), c.gc, c.ge, np.float32, True, True)
        check_construction(o["radii"], live, n)
        assert min(oracle_row_share(o, live, n, k_cols)) >= MIN_SHARE
        views = big["d_views"].copy()
        views[:, 35:37] = 0.0  # (the tan-fov columns have no analytic oracle: they rest on (a) and (b))
        hip = dict(big["res"], grads=dict(big["res"]["grads"], views=views))
        res = dict(hip=hip, oracle=o)
        fig["camera_worst"] = parity_checks.check_camera_grads(res)
        mg = parity_checks.check_grads(res, c.cfg)
        fig["grads_worst"] = max(x for k, x in mg.items() if k.endswith("_rel_l2"))
        print(name, "oracle", {k: f"{fig[k]:.3g}" for k in ("camera_worst", "grads_worst")})
    else:
        o = gpu_util.run_oracle(*c.args())
        check_construction(o["radii"], live, n)
    return fig, bigs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["below", "edge", "model", "two_trips", "fov", "small"])
def test_full_gradient_reduction(name):
    fig, _ = _case(name, oracle=True)
    assert 0 < fig["camera_worst"] < parity_checks.TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["z_one", "z_two", "small_z"])
def test_depth_only_reduction(name):
    _, (big,) = _case(name, oracle=False)
    assert (big["d_views"][:, list(Z_SLOTS)] != 0).all()


@pytest.mark.gpu
def test_model_size_deterministic_runs_give_equal_bits():
    fig, (r1, r2) = _case("model_det", oracle=True, runs=2)
    assert 0 < fig["camera_worst"] < parity_checks.TOL
    assert fig["twin_widened"] == 0.0  # fixed-point cotangent rows: the twin's two runs carry the same rows
    for k in ("d_views", "level0", "level1"):
        assert np.array_equal(_bits(r1[k]), _bits(r2[k])), k
