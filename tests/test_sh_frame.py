"""Harmonics given in their group's frame (GSR_FLAG_SH_IN_FRAME, rasterize_views(sh_frame=...), GaussianAdapter(fuse_sh_rotation=
True)): the direction identity behind it, the adapter's fused output, the torch fallback of a backend without the capability, and
the host-side checks of the binding and the C ABI.  No GPU: the kernels themselves are checked in tests/test_gpu_sh_frame.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pf3plat_amd
from pf3plat_amd import _lib, rasterizer
from pf3plat_amd.adapter import GaussianAdapter, GaussianAdapterCfg
from pf3plat_amd.sh_rotation import direction_frame, rotate_sh, sh_basis
from tests.util import rel_l2

FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "adapter_fixtures.npz"))
t = lambda k: torch.tensor(FIX[k])


def _proper_rotations(n, seed):
    q = torch.linalg.qr(torch.randn(n, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)))[0]
    return q * torch.det(q)[:, None, None]  # (an odd number of flipped signs: det -1 -> +1)


@pytest.mark.parametrize("basis", ["rasterizer", "e3nn"])
@pytest.mark.parametrize("degree", [0, 1, 2, 3, 4])
def test_rotated_coefficients_equal_unrotated_ones_at_the_frame_direction(basis, degree):
    """B(d) . rotate_sh(c, F, basis) == B(G^T d) . c with G = direction_frame(F, basis), in fp64."""
    r = _proper_rotations(64, degree)
    assert torch.allclose(torch.det(r), torch.ones(64, dtype=torch.float64))
    g = torch.Generator().manual_seed(10 + degree)
    c = torch.randn(64, 3, (degree + 1) ** 2, dtype=torch.float64, generator=g)
    d = torch.nn.functional.normalize(torch.randn(64, 5, 3, dtype=torch.float64, generator=g), dim=-1)
    lhs = torch.einsum("vpk,vck->vpc", sh_basis(d, degree), rotate_sh(c, r[:, None], basis=basis))
    local = torch.einsum("vjk,vpj->vpk", direction_frame(r, basis), d)  # G^T d
    rhs = torch.einsum("vpk,vck->vpc", sh_basis(local, degree), c)
    assert (lhs - rhs).abs().max().item() < 1e-12


def _cfg():
    lo, hi, deg = FIX["B_cfg"]
    return GaussianAdapterCfg(float(lo), float(hi), int(deg))


def _adapt(ad, ext=None):
    hw = tuple(int(x) for x in FIX["B_hw"])
    raw = t("B_in_raw").requires_grad_(True)
    ext = t("B_in_ext") if ext is None else ext
    out = ad.forward(ext[:, :, None], t("B_in_intr")[:, :, None], t("B_in_coords"), t("B_in_depths"), t("B_in_opac"), raw, hw)
    return out, raw


@pytest.mark.parametrize("basis", ["e3nn", "rasterizer"])
def test_fused_adapter_matches_the_default_adapter(basis):
    default = _adapt(GaussianAdapter(_cfg(), rotate_sh=lambda sh, r: rotate_sh(sh, r, basis=basis)))[0]
    fused = _adapt(GaussianAdapter(_cfg(), fuse_sh_rotation=True, sh_basis=basis))[0]
    assert default.sh_frame is None and fused.sh_frame == basis
    for name in ("means", "scales", "rotations", "opacities", "frames"):
        assert torch.equal(getattr(fused, name), getattr(default, name)), name
    assert torch.allclose(fused.world_harmonics, default.harmonics, atol=1e-6, rtol=1e-5)
    assert not torch.allclose(fused.harmonics, default.harmonics, atol=1e-3)  # the fused harmonics are NOT in world space
    assert torch.equal(default.world_harmonics, default.harmonics)
    g = fused.for_decoder()
    assert g.sh_frame == basis and g.clone().sh_frame == basis and default.for_decoder().sh_frame is None
    assert torch.equal(g.harmonics, fused.harmonics.reshape(g.harmonics.shape))
    assert fused.for_decoder(views=(0, -1)).sh_frame == basis


def test_fused_adapter_keeps_the_determinant_rule():
    """A frame with det -1 (a QR factor, a mirrored camera): rotate_sh uses no rotation at all (reference sh_rotation.py:20-21),
    and the fused adapter says "already world space" (sh_frame None) with the same, unrotated, harmonics."""
    ext = t("B_in_ext").clone()
    ext[:, -1, :3, 0] *= -1
    assert torch.det(ext[0, -1, :3, :3]) < 0
    default = _adapt(GaussianAdapter(_cfg()), ext)[0]
    fused = _adapt(GaussianAdapter(_cfg(), fuse_sh_rotation=True), ext)[0]
    assert fused.sh_frame is None and fused.for_decoder().sh_frame is None
    assert torch.equal(fused.harmonics, default.harmonics) and torch.equal(fused.world_harmonics, default.harmonics)
    with pytest.raises(ValueError, match="sh_basis"):
        GaussianAdapter(_cfg(), fuse_sh_rotation=True, sh_basis="wigner")


def _scene_and_weights():
    from pf3plat_amd import synthetic

    sc = synthetic.make_scene(3, 8, (24, 32), num_views=2)  # (only its cameras are used)
    w = torch.rand((1, 2, 3, 24, 32), generator=torch.Generator().manual_seed(5))
    wd = torch.rand((1, 2, 24, 32), generator=torch.Generator().manual_seed(6)) * 0.05
    return sc, w, wd


@pytest.mark.parametrize("basis", ["e3nn", "rasterizer"])
def test_decoder_renders_the_fused_adapter_like_the_default_one(oracle_backend, basis):
    """Through a backend without the capability (the CPU oracle): the Python layer rotates in torch; colour, depth and the gradient
    w.r.t. the adapter's raw inputs equal the default adapter's (tolerances of test_adapter.py's scale / rotation test)."""
    assert not getattr(oracle_backend, "sh_frame", False)
    sc, w, wd = _scene_and_weights()
    dec = pf3plat_amd.DecoderSplattingCUDA()
    res = []
    for fused in (True, False):
        ad = GaussianAdapter(_cfg(), fuse_sh_rotation=True, sh_basis=basis) if fused else \
            GaussianAdapter(_cfg(), rotate_sh=lambda sh, r: rotate_sh(sh, r, basis=basis))
        out, raw = _adapt(ad)
        g = out.for_decoder()
        assert g.sh_frame == (basis if fused else None)
        o = dec.forward(g, sc.extrinsics, sc.intrinsics, sc.near, sc.far, (24, 32), depth_mode="depth")
        ((o.color * w).sum() + (o.depth * wd).sum()).backward()
        res.append((o.color.detach().numpy(), o.depth.detach().numpy(), raw.grad.numpy()))
    assert rel_l2(res[0][0], res[1][0]) < 1e-6 and rel_l2(res[0][1], res[1][1]) < 1e-6
    assert np.abs(res[1][2][..., 7:]).max() > 0 and rel_l2(res[0][2], res[1][2]) < 2e-5


def _call_args(n=64, sets=1, frames=2):
    g = torch.Generator().manual_seed(3)
    means = torch.randn(sets, n, 3, generator=g)
    records = torch.randn(sets, n, 7, generator=g)
    opac = torch.rand(sets, n, generator=g)
    sh = torch.randn(sets, n, 3, 25, generator=g)
    fr = torch.linalg.qr(torch.randn(sets, frames, 3, 3, generator=g))[0]
    return means, records, opac, sh, torch.zeros(sets, 48), fr


def test_sh_frame_argument_checks(oracle_backend):
    means, records, opac, sh, vb, fr = _call_args()
    kw = dict(image_shape=(16, 16), sh_degree=4, views_per_set=1, sh_planar=True)
    with pytest.raises(ValueError, match="sh_frame must be"):
        rasterizer.rasterize_views(means, records, opac, sh, vb, use_sh=True, scale_rot=True, frames=fr, sh_frame="world", **kw)
    with pytest.raises(ValueError, match="scale_rot=True and `frames`"):
        rasterizer.rasterize_views(means, records, opac, sh, vb, use_sh=True, scale_rot=True, sh_frame="e3nn", **kw)
    with pytest.raises(ValueError, match="scale_rot=True and `frames`"):
        cov = torch.eye(3).expand(1, 64, 3, 3)
        rasterizer.rasterize_views(means, cov, opac, sh, vb, use_sh=True, cov_3x3=True, sh_frame="rasterizer", **kw)
    with pytest.raises(ValueError, match="use_sh=True"):
        rasterizer.rasterize_views(means, records, opac, sh[..., 0], vb, use_sh=False, scale_rot=True, frames=fr, sh_frame="e3nn", **kw)
    # the binding states the flags: GSR_FLAG_SH_IN_FRAME, with GSR_FLAG_SH_FRAME_E3NN for "e3nn"
    ext = _lib.load_torch_ext()
    for code, bits in ((0, 0), (1, _lib.FLAG_SH_IN_FRAME), (2, _lib.FLAG_SH_IN_FRAME | _lib.FLAG_SH_FRAME_E3NN)):
        cfg = ext.prepare_call(means, records, opac, sh, vb, 16, 16, 4, True, 1, None, None, 4, True, False, 0, False, False, -1, True, fr,
                               1, code)[0]
        assert isinstance(cfg, rasterizer.RasterConfig)
        assert cfg.flags & (_lib.FLAG_SH_IN_FRAME | _lib.FLAG_SH_FRAME_E3NN) == bits
        assert cfg.alpha is False and cfg.scale_rot is True


def _dims(flags, sh_coeffs=25):
    return rasterizer.HipBackend._dims(rasterizer.RasterConfig(1, 1, 1, 128, 16, 16, 4, sh_coeffs, 4, False, flags, True), 4096)


def test_c_entry_points_reject_the_bits_outside_the_scale_rotation_form():
    """Host-side checks of the loaded library (no launch, no GPU): the bits only go with the scale / rotation launches, frames and
    harmonics; the sizing helpers take the dims without them."""
    lib = _lib.load()
    z = ctypes.c_size_t()
    frame, e3nn = _lib.FLAG_SH_IN_FRAME, _lib.FLAG_SH_FRAME_E3NN
    sizes = lambda d: lib.gsr_workspace_sizes(ctypes.byref(d), ctypes.byref(z), ctypes.byref(z), ctypes.byref(z))
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p).value

    def forward_ex(d, *opt):  # opt: frames, num_frames, scale_rot; nothing = NULL options
        return lib.gsr_forward_ex(ctypes.byref(d), *([None] * 12), ctypes.byref(_lib.GsrForwardOptions(*opt)) if opt else None, None)

    def backward_ex(d, *opt):
        return lib.gsr_backward_ex(ctypes.byref(d), *([None] * 18), ctypes.byref(_lib.GsrBackwardOptions(*opt)) if opt else None, None)

    assert sizes(_dims(0)) == 0
    for bits in (frame, frame | e3nn, e3nn):
        d = _dims(bits)
        assert sizes(d) == -1, hex(bits)
        assert lib.gsr_backward_scratch_bytes(ctypes.byref(d)) == 0 and lib.gsr_pose_partials_bytes(ctypes.byref(d)) == 0
        assert lib.gsr_forward(ctypes.byref(d), *([None] * 13)) == -1
        assert lib.gsr_backward(ctypes.byref(d), *([None] * 19)) == -1
        for ex in (forward_ex, backward_ex):
            assert ex(d) == -1  # without options
            assert ex(d, None, 0, 1) == -1  # scale / rotation form without frames
            assert ex(d, fake, 2, 0) == -1  # options, frames even, but not the scale / rotation form
    # the e3nn bit alone, and the bits on colours that are not harmonics, even with frames
    for d in (_dims(e3nn), _dims(frame, sh_coeffs=0)):
        assert forward_ex(d, fake, 2, 1) == -1
        assert backward_ex(d, fake, 2, 1) == -1
