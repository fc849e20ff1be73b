"""The raster backward at the cotangent magnitudes training hands it, on the MI355X against the CPU oracle.

Every other GPU test feeds the backward image gradients of order one.  A loss that is a mean over the pixels of a batch hands back
weight / count per pixel: about 3e-7 at 3 views x 3 x 256 x 256 with a residual of 0.1, about 2e-8 at the reference's batch of 14
scenes; a loss-scaled sum hands back 2^20 and more.  The backward is linear in its cotangents, so none of that may show in the
relative error - and the deterministic mode (GSR_FLAG_DETERMINISTIC: 64-bit fixed-point sums) only has that property because its
sums are kept in units of each view's largest cotangent (gsr_hip.hip det_max_words).

The bound is parity_checks.TOL (1e-4, rel-L2 per tensor, nothing set aside) against the fp32 oracle: rel-L2 is scale-free, so it is
the same number at every scale.  Every scale is a power of two: scaling a cotangent by it is exact in fp32, and so is comparing
grads(s g) / s with grads(g).  The base case (seed 71) was chosen on the CPU: the fp32 oracle against the fp64 oracle passes
check_grads with nothing set aside and no flipped pixel at s = 2^-26, 2^-19, 1 and 2^20 (worst tensor 2.9e-6, camera blocks 7.9e-6).
The measured figures of both modes, before and after the per-view unit, are in docs/PARITY.md, section 8."""
import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, losses, rasterizer, synthetic
from pf3plat_amd.rasterizer import RasterConfig
from tests import gpu_util, parity_checks
from tests.test_alpha_gpu import _rand_grads, case_two_sets, check_all, hip_alpha, oracle_alpha
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEPTH = 1 << 4  # GSR_FLAG_EXTRA_MODE(GSR_EXTRA_DEPTH)
DET = _lib.FLAG_DETERMINISTIC
MODES = {"default": 0, "deterministic": DET}
GRADS = ("means", "cov6", "opac", "colors", "means2d", "views")
N, HW = 3000, (64, 64)


class _Base:
    """make_scene(71, 3000, (64, 64), V views, near = 1.5), degree-4 harmonics, built-in depth; unit cotangents 2 N(0, delta) in fp32."""

    def __init__(self, views):
        sc = synthetic.make_scene(71, N, HW, num_views=views, near=1.5)
        self.views = views
        self.args = gpu_util.scene_tensors(sc)
        self.vb = gpu_util.scene_viewbuf(sc)
        self._unit, self._oracle, self._hip = {}, {}, {}

    def cfg(self, flags=0):
        return RasterConfig(self.views, 1, self.views, N, *HW, 4, 25, 4, True, DEPTH | flags)

    def unit(self, delta):
        if delta not in self._unit:
            rng = np.random.default_rng(71)
            self._unit[delta] = tuple(torch.tensor((2.0 * rng.normal(0.0, delta, shape)).astype(np.float32))
                                      for shape in ((self.views, 3, *HW), (self.views, *HW)))
        return self._unit[delta]

    def cotangents(self, delta, s):
        """s: one power of two, or one per view."""
        gc, ge = self.unit(delta)
        sv = torch.tensor(np.broadcast_to(np.asarray(s, np.float32), (self.views,)).copy())
        return gc * sv[:, None, None, None], ge * sv[:, None, None]

    def oracle(self, delta, s):
        """The fp32 oracle's own run at that scale, computed once and shared by both modes."""
        key = (delta, tuple(np.broadcast_to(np.asarray(s, np.float64), (self.views,))))
        if key not in self._oracle:
            gc, ge = self.cotangents(delta, s)
            self._oracle[key] = gpu_util.run_oracle(self.cfg(), self.vb, *self.args, None, gc, ge, want_views=True)
        return self._oracle[key]

    def hip(self, mode, delta, s, keep=False):
        key = (mode, delta, s)
        if keep and key in self._hip:
            return self._hip[key]
        gc, ge = self.cotangents(delta, s)
        out = gpu_util.run_hip(self.cfg(MODES[mode]), self.vb, *self.args, None, gc, ge, want_views=True)
        assert not out["status"]["overflow"]
        if keep:
            self._hip[key] = out
        return out


@pytest.fixture(scope="module")
def base():
    return _Base(2)


@pytest.fixture(scope="module")
def three_views():
    return _Base(3)


def _check(cfg, h, o):
    """check_grads with nothing set aside, and the camera blocks; prints every figure before it asserts."""
    res = dict(hip=h, oracle=o)
    print({k: f"{rel_l2(h['grads'][k], o['grads'][k]):.3e}" for k in GRADS})
    m = parity_checks.check_grads(res, cfg)
    parity_checks.assert_nothing_set_aside(m)
    worst = parity_checks.check_camera_grads(res)
    print("camera blocks, worst:", f"{worst:.3e}")
    return m


# ---- parity at every scale ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta,s", [(0.1, 2.0 ** -26), (0.1, 2.0 ** -19), (0.1, 2.0 ** -12), (0.1, 1.0), (0.1, 2.0 ** 12),
                                     (0.1, 2.0 ** 20), (0.01, 2.0 ** -19)])
@pytest.mark.parametrize("mode", list(MODES))
def test_gradients_match_the_oracle_at_every_cotangent_scale(base, mode, delta, s):
    h = base.hip(mode, delta, s, keep=(delta == 0.1 and s == 1.0))
    o = base.oracle(delta, s)
    assert np.array_equal(h["color"], base.hip(mode, 0.1, 1.0, keep=True)["color"])  # (the forward does not know the cotangents)
    m = _check(base.cfg(), h, o)
    assert m["means_norm"] > 0 and m["views_norm"] > 0


# ---- homogeneity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2.0 ** -24, 2.0 ** -12, 2.0 ** 12])
@pytest.mark.parametrize("mode", list(MODES))
def test_backward_is_homogeneous_in_its_cotangents(base, mode, s):
    """grads(s g) / s against grads(g), the same mode, per tensor (s a power of two: the division is exact).  Deterministic: rel-L2 <=
    1e-6 (16 fp32 roundings, the floor of docs/PARITY.md; with sums in units of the view's largest cotangent the integer sums are
    the same integers and the expected value is exactly 0 - whether the bits agree is printed).  Default: the run-to-run bound of
    test_forward_is_deterministic_and_backward_nearly, max-abs <= 1e-5 max|grad| (fp32 atomics, order-dependent rounding only).
    Both: the support of the screen-space gradient does not move - no contribution is rounded away at any scale."""
    one, scaled = base.hip(mode, 0.1, 1.0, keep=True)["grads"], base.hip(mode, 0.1, s)["grads"]
    same_bits = {}
    for k in GRADS:
        a, b = one[k], scaled[k] / np.float32(s)
        assert np.isfinite(scaled[k]).all() and a.any(), k
        same_bits[k] = bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
        err, worst = rel_l2(b, a), float(np.abs(b.astype(np.float64) - a).max() / np.abs(a).max())
        print(f"{mode} s = 2^{int(np.log2(s))} {k}: rel-L2 {err:.3e}, max-abs / max|grad| {worst:.3e}, same bits {same_bits[k]}")
    for k in GRADS:
        a, b = one[k], scaled[k] / np.float32(s)
        if mode == "deterministic":
            assert rel_l2(b, a) <= 1e-6, (k, rel_l2(b, a))
        else:
            assert np.abs(b.astype(np.float64) - a).max() <= 1e-5 * np.abs(a).max(), k
    assert np.array_equal(one["means2d"] != 0, scaled["means2d"] != 0)


# ---- views of unequal magnitude ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_views_of_unequal_cotangent_magnitude_in_one_call(three_views, mode):
    """Three views of one set, cotangents scaled 1, 2^-20 and exactly 0: the faint view keeps its own relative precision next to the
    loud one (its screen-space gradient is a tensor of its own; in the summed tensors it is below the loud view's rounding), and
    the view without a loss contributes exact zeros."""
    s = (1.0, 2.0 ** -20, 0.0)
    h, o = three_views.hip(mode, 0.1, s), three_views.oracle(0.1, s)
    for k in GRADS:
        assert np.isfinite(h["grads"][k]).all(), k
    for v in (0, 1):
        err = rel_l2(h["grads"]["means2d"][v], o["grads"]["means2d"][v])
        print(f"{mode} view {v} means2d rel-L2 {err:.3e}")
    for v in (0, 1):
        assert o["grads"]["means2d"][v].any()
        assert rel_l2(h["grads"]["means2d"][v], o["grads"]["means2d"][v]) < parity_checks.TOL, v
    assert not h["grads"]["means2d"][2].any() and not h["grads"]["views"][2].any()
    _check(three_views.cfg(), h, o)


def test_all_zero_cotangents_give_exact_zeros_in_deterministic_mode(base):
    h = base.hip("deterministic", 0.1, 0.0)
    for k in GRADS:
        assert np.isfinite(h["grads"][k]).all() and not h["grads"][k].any(), k


# ---- the other options of the deterministic instances -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_sets_faint():
    case = case_two_sets()
    gc, ge, ga = (t * 2.0 ** -19 for t in _rand_grads(case[0], 2))
    return gc, ge, ga, oracle_alpha(case, gc, ge, ga)


@pytest.mark.parametrize("follows", [False, True])
def test_deterministic_scale_rotation_records_planar_harmonics_depth_and_alpha_at_2_to_minus_19(two_sets_faint, follows):
    """tests/test_alpha_gpu.py's two sets x three views (records in frames, planar harmonics, built-in depth, an alpha cotangent) with
    every cotangent scaled by 2^-19, the accumulator rows in the caller's scratch and inside geom (GSR_FLAG_BACKWARD_FOLLOWS)."""
    gc, ge, ga, o = two_sets_faint
    case = case_two_sets(DET | (_lib.FLAG_BACKWARD_FOLLOWS if follows else 0))
    check_all(case, hip_alpha(case, gc, ge, ga, follows=follows), o)


# ---- batch = single calls -----------------------------------------------------------------------------------------------------------
def test_small_batch_with_per_scene_cotangent_scales_equals_its_single_scene_calls_bit_for_bit():
    """3 scenes x 2 views, cotangents of the scenes scaled 1, 2^-10 and 2^-20, deterministic: one batched call returns the bits of the
    three single-scene calls (the unit of the fixed-point sums belongs to a view, not to a launch)."""
    b_sets, n, hw = 3, 2000, (48, 48)
    scs = [synthetic.make_scene(90 + b, n, hw, num_views=2) for b in range(b_sets)]
    parts = [gpu_util.scene_tensors(sc) for sc in scs]
    vbs = [gpu_util.scene_viewbuf(sc) for sc in scs]
    rng = np.random.default_rng(90)
    sv = torch.tensor(np.repeat(np.float32([1.0, 2.0 ** -10, 2.0 ** -20]), 2))
    gc = torch.tensor((2.0 * rng.normal(0, 0.1, (2 * b_sets, 3, *hw))).astype(np.float32)) * sv[:, None, None, None]
    ge = torch.tensor((2.0 * rng.normal(0, 0.1, (2 * b_sets, *hw))).astype(np.float32)) * sv[:, None, None]
    cfg_b = RasterConfig(2 * b_sets, b_sets, 2, n, *hw, 4, 25, 4, True, DEPTH | DET)
    whole = gpu_util.run_hip(cfg_b, torch.cat(vbs), *(torch.cat([p[k] for p in parts]) for k in range(4)), None, gc, ge, want_views=True)
    assert not whole["status"]["overflow"]
    cfg_1 = RasterConfig(2, 1, 2, n, *hw, 4, 25, 4, True, DEPTH | DET)
    for b in range(b_sets):
        v = slice(2 * b, 2 * b + 2)
        one = gpu_util.run_hip(cfg_1, vbs[b], *parts[b], None, gc[v], ge[v], want_views=True)
        assert np.array_equal(whole["color"][v].view(np.uint32), one["color"].view(np.uint32)), b
        for name in ("means", "cov6", "opac", "colors"):
            assert one["grads"][name].any(), (b, name)
            assert np.array_equal(whole["grads"][name][b: b + 1].view(np.uint32), one["grads"][name].view(np.uint32)), (b, name)
        for name in ("means2d", "views"):
            assert np.array_equal(whole["grads"][name][v].view(np.uint32), one["grads"][name].view(np.uint32)), (b, name)


# ---- the real composition -----------------------------------------------------------------------------------------------------------
def test_photometric_loss_through_rasterize_views_under_deterministic_algorithms(base):
    """What a training step composes: torch.use_deterministic_algorithms(True) -> rasterize_views(deterministic=None) picks the fixed-point
    backward -> losses.photometric_loss(pred, target, 1.0, 0.2) (a mean: weight / count per pixel) -> backward, the loss scaled by a
    further 2^-6 to stand for the pixel count of 3 views x 3 x 256 x 256.  The cotangent the loss produced goes to the oracle."""
    dev = torch.device("cuda:0")
    means, cov6, opac, colors = base.args
    g = torch.Generator().manual_seed(71)
    other = colors * (1.0 + 0.02 * torch.randn(colors.shape, generator=g))
    kw = dict(image_shape=HW, sh_degree=4, use_sh=True, views_per_set=2, deterministic=None)
    vb = base.vb.to(dev)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        with torch.no_grad():
            target = rasterizer.rasterize_views(means.to(dev), cov6.to(dev), opac.to(dev), other.to(dev), vb, **kw)[0]

        def step():
            leaves = [t.to(dev).requires_grad_(True) for t in (means, cov6, opac, colors)]
            pred = rasterizer.rasterize_views(*leaves, vb, **kw)[0]
            pred.retain_grad()
            (losses.photometric_loss(pred, target, 1.0, 0.2)[0] * 2.0 ** -6).backward()
            return pred, [t.grad.cpu().numpy() for t in leaves]

        pred, grads = step()
        _, again = step()
    finally:
        torch.use_deterministic_algorithms(was)
    for a, b in zip(grads, again):  # (the fixed-point backward was the one selected)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    g_pred = pred.grad.cpu()
    peak = float(g_pred.abs().max())
    print(f"largest cotangent of the loss: {peak:.3e}")
    assert 0 < peak < 1e-5
    cfg = RasterConfig(2, 1, 2, N, *HW, 4, 25, 4, False, 0)
    o = gpu_util.run_oracle(cfg, base.vb, means, cov6, opac, colors, None, g_pred, None, want_means2d=False)
    names = ("means", "cov6", "opac", "colors")
    h = dict(color=pred.detach().cpu().numpy(), grads=dict(zip(names, grads)))
    o = dict(o, grads={k: o["grads"][k] for k in names})
    print({k: f"{rel_l2(h['grads'][k], o['grads'][k]):.3e}" for k in names})
    parity_checks.assert_nothing_set_aside(parity_checks.check_grads(dict(hip=h, oracle=o), cfg))
