"""The scale / rotation case generator of the parity tests (tests/fuzz_cases.py draw_sr_case) and the oracle side of
tests/gpu_util.run_both in that form - no GPU: a case is a pure function of (seed, index), draw_case's own sequence has not moved,
every frames tensor is one the binding accepts, and the oracle side (harmonics rotated to world space in fp64, gradient pulled back
through the rotation) agrees with `rasterize_views` on the oracle backend, which takes its torch-rotation fallback for sh_frame."""
import numpy as np
import pytest
import torch

from pf3plat_amd import _lib, rasterizer
from tests import fuzz_cases, gpu_util
from tests.oracle_backend import OracleBackend
from tests.util import install_backend, rel_l2


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_sr_case_is_a_pure_function_of_seed_and_index():
    for seed, index in ((11, 0), (11, 5), (3, 26)):
        d1, in1 = fuzz_cases.named_sr_case(seed, index)
        d2, in2 = fuzz_cases.named_sr_case(seed, index)
        assert d1 == d2 and _same(in1, in2), (seed, index)


def test_sr_case_without_building_leaves_the_generator_where_building_does():
    a, b = np.random.default_rng(11), np.random.default_rng(11)
    for k in range(12):
        da, ia = fuzz_cases.draw_sr_case(a, build=(k % 3 == 0))
        db, ib = fuzz_cases.draw_sr_case(b, build=False)
        assert da == db and ib is None, k
        assert a.bit_generator.state == b.bit_generator.state, k
        assert (ia is None) == (k % 3 != 0)


def test_draw_case_sequence_did_not_move():
    """Two of the named WORST_CASES, pinned: the old generator still names the same shapes."""
    assert (8, 275) in fuzz_cases.WORST_CASES and (4, 363) in fuzz_cases.WORST_CASES
    pinned = {
        (8, 275): dict(n=63, hw=(66, 89), sets=2, vps=1, d_sh=16, use_sh=True, extra=False, windowed=False, seed=243015486, cap=None,
                       planar=False, cov33=False, emode=0, follows=True, det=False),
        (4, 363): dict(n=65, hw=(128, 8), sets=2, vps=2, d_sh=16, use_sh=False, extra=False, windowed=False, seed=153803712, cap=None,
                       planar=False, cov33=True, emode=0, follows=True, det=False),
    }
    for (seed, index), want in pinned.items():
        rng = np.random.default_rng(seed)
        for _ in range(index):
            fuzz_cases.draw_case(rng, build=False)
        assert fuzz_cases.draw_case(rng, build=False)[0] == want, (seed, index)


def test_drawn_frames_pass_the_bindings_shape_rule_and_are_proper_rotations_per_set():
    frames_arg = _lib.load_torch_ext().frames_arg
    rng = np.random.default_rng(11)  # the sequence tests/test_gpu_scale_rot_parity.py runs
    kinds = set()
    for k in range(24):
        desc, (cfg, vb, means, records, opac, colors, extra, gc, ge, cap, frames, sh_frame, want_views) = fuzz_cases.draw_sr_case(rng)
        s, n = cfg.num_sets, cfg.num_gaussians
        assert cfg.scale_rot and records.shape == (s, n, 7) and means.shape == (s, n, 3) and vb.shape[0] == cfg.num_views
        assert not cfg.flags & gpu_util.SH_FRAME_BITS["e3nn"]  # (the SH-frame bits are added by run_both from sh_frame)
        if sh_frame is not None:
            assert frames is not None and cfg.sh_coeffs >= (cfg.sh_degree + 1) ** 2 and cfg.sh_coeffs > 0, k
        if frames is None:
            assert desc["frames"] == 0
            continue
        fr, nf = frames_arg(cfg, frames)
        assert nf == frames.shape[1] == desc["frames"] and n % nf == 0 and tuple(fr.shape) == (s, nf, 3, 3), k
        f64 = frames.double()
        assert torch.allclose(f64 @ f64.transpose(-1, -2), torch.eye(3, dtype=torch.float64).expand_as(f64), atol=1e-5), k
        assert torch.allclose(torch.det(f64), torch.ones(f64.shape[:2], dtype=torch.float64), atol=1e-5), k
        for a in range(s):
            for b in range(a):
                assert not torch.equal(frames[a], frames[b]), (k, a, b)
        kinds.add("one" if nf == 1 else "each" if nf == n else "straddle" if (n // nf) % 64 else "other")
    assert {"one", "each", "straddle"} <= kinds, kinds


@pytest.mark.parametrize("seed, index", [(0, 33), (4, 496)])
def test_oracle_side_with_frames_equals_rasterize_views_on_the_oracle_backend(seed, index):
    """A tiny drawn case (N <= 64, images <= 16 px, several scenes, harmonics in per-Gaussian / straddling frames) through
    gpu_util.run_oracle, against `rasterize_views(..., sh_frame=)` with the oracle backend installed: the same image, and the same
    gradients of means, records, opacities and frame harmonics (autograd through the torch rotation fallback)."""
    desc, (cfg, vb, means, records, opac, colors, extra, gc, ge, cap, frames, sh_frame, want_views) = fuzz_cases.named_sr_case(seed, index)
    assert 0 < cfg.num_gaussians <= 64 and max(cfg.height, cfg.width) <= 16 and sh_frame is not None and cfg.sh_degree >= 1
    res = gpu_util.run_oracle(cfg, vb, means, records, opac, colors, extra, gc, ge, want_means2d=False, frames=frames, sh_frame=sh_frame)
    emode = (cfg.flags >> 4) & 7
    leaves = [t.clone().requires_grad_(True) for t in (means, records, opac, colors)]
    ex = extra.clone().requires_grad_(True) if extra is not None else None
    old = install_backend(OracleBackend())
    try:
        color, ext_img, _ = rasterizer.rasterize_views(
            *leaves, vb, image_shape=(cfg.height, cfg.width), sh_degree=cfg.sh_degree, use_sh=True, views_per_set=cfg.views_per_set,
            extra=ex, max_sh_eval=cfg.max_sh_eval, sh_planar=bool(cfg.flags & _lib.FLAG_SH_PLANAR),
            extra_mode={v: k for k, v in rasterizer.EXTRA_MODES.items()}[emode] if emode else None, deterministic=desc["det"],
            scale_rot=True, frames=frames, sh_frame=sh_frame)
        loss = (color * gc).sum() + ((ext_img * ge).sum() if ext_img is not None else 0)
        grads = torch.autograd.grad(loss, leaves)
    finally:
        install_backend(old)
    assert np.abs(res["color"]).max() > 0.05
    assert rel_l2(color.detach().numpy(), res["color"]) < 1e-5
    if cfg.has_extra:
        assert rel_l2(ext_img.detach().numpy(), res["extra"]) < 1e-5
    for name, g in zip(("means", "cov6", "opac", "colors"), grads):
        assert np.abs(res["grads"][name]).max() > 0, name
        assert rel_l2(g.numpy(), res["grads"][name]) < 1e-4, name
    # the pull-back did something: the frame harmonics' gradient is not the world harmonics' one
    world = gpu_util.run_oracle(cfg, vb, means, records, opac, rasterizer._rotate_in_frames(
        colors.double(), frames.double(), bool(cfg.flags & _lib.FLAG_SH_PLANAR), sh_frame).float(), extra, gc, ge, want_means2d=False,
        frames=frames)
    assert rel_l2(world["color"], res["color"]) < 1e-5
    assert rel_l2(world["grads"]["colors"], res["grads"]["colors"]) > 1e-2


def test_kernel_order_covariance_is_the_adapters_formula():
    """gpu_util.cov6_in_kernel_order (what the oracle side rasterizes in the scale / rotation form) against oracle/adapter.py's covariance
    in fp64 - the formula pinned to the reference by tests/golden/adapter_fixtures.npz - with and without frames, F = 1 / N / straddling."""
    from oracle import adapter

    for seed, index in ((0, 33), (4, 496), (11, 16), (11, 48)):
        desc, (cfg, vb, means, records, opac, colors, extra, gc, ge, cap, frames, sh_frame, want_views) = fuzz_cases.named_sr_case(seed, index)
        for fr in (frames, None):
            got = gpu_util.cov6_in_kernel_order(records, fr).double()
            want = adapter.cov6_from_scale_rotation(records.double(), None if fr is None else fr.double())
            scale = want[..., [0, 3, 5]].abs().amax(-1, keepdim=True)  # per Gaussian: the largest variance
            assert float(((got - want).abs() / scale).max()) < 1e-5, (seed, index, fr is None)
